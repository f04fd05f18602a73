/* clip_demo.c — one CLIPPED optimizer step from plain C: no Python, no torch.  Build like optim_demo.c
 * (tests/test_cabi_clip.py does it and runs it on the GPU box).
 * A small model (d 128, 2 heads of 64, 1 layer, no positional table) whose parameters and gradients are an integer hash
 * of (tensor, element) - the test regenerates the same numbers - then
 *   vs_grad_norm(max_norm = 1)  ->  vs_adam_step(grad_scale = out + 2)
 * with a device-side loss scale of 1024 on the gradients: the norm launches write grad_scale / clip_coef into out[2] and
 * the update kernel divides by it; the gradients themselves are never rewritten.  A second measurement with a generous
 * max_norm must give clip_coef == 1 and hand the scale through bit for bit.
 * Prints "OK", then as bit patterns: norm, clip_coef, divisor, embed_w[PROBE] after the step, the unclipped clip_coef and
 * divisor, and the first gradient element (unchanged). */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vs_optim.h"

enum { D = 128, H = 2, L = 1, DIN = 1024, NT = 4 + 16 * L, PROBE = 54321 };

static float hval(uint32_t tensor, uint32_t i) {
    uint32_t h = i * 2654435761u + tensor * 40503u + 12345u;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    return (float)(h >> 8) / 8388608.0f - 1.0f;          /* [-1, 1), every step exact */
}
static float *dev_hash(uint32_t tensor, size_t n, float scale) {
    float *h = (float *)malloc(n * sizeof(float)), *d = NULL;
    for (size_t i = 0; i < n; ++i) h[i] = hval(tensor, (uint32_t)i) * scale;
    if (hipMalloc((void **)&d, n * sizeof(float)) != hipSuccess) exit(2);
    hipMemcpy(d, h, n * sizeof(float), hipMemcpyHostToDevice);
    free(h);
    return d;
}
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
#define CHECK(call) do { int rc_ = (call); if (rc_ != VS_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, vs_last_error()); return 1; } } while (0)
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

int main(void) {
    /* element counts in vs_model_params order (include/vs_optim.h: vs_adam_state_field) */
    size_t n[NT];
    const size_t layer_n[16] = {D * D, D, D * D, D, D * D, D, D * D, D, D, D, 4 * D * D, 4 * D, 4 * D * D, D, D, D};
    n[0] = (size_t)D * DIN; n[1] = D;
    for (int j = 0; j < 16; ++j) n[2 + j] = layer_n[j];
    n[2 + 16 * L] = D; n[3 + 16 * L] = 1;
    float *p[NT], *g[NT];
    vs_grad_tensor table[NT];
    for (int i = 0; i < NT; ++i) {
        p[i] = dev_hash((uint32_t)i, n[i], 0.125f);
        g[i] = dev_hash(100u + (uint32_t)i, n[i], 16.0f);            /* "scaled" gradients: 1024 x (1 / 64) */
        table[i].g = g[i]; table[i].n = n[i];
    }
    vs_layer_params layers[L];
    vs_layer_grads glayers[L];
    memcpy(&layers[0], &p[2], 16 * sizeof(float *));                 /* 16 pointers in declaration order */
    memcpy(&glayers[0], &g[2], 16 * sizeof(float *));
    vs_model_params P;
    P.embed_w = p[0]; P.embed_b = p[1]; P.pos_embedding = NULL; P.layers = layers; P.final_w = p[2 + 16 * L]; P.final_b = p[3 + 16 * L];
    vs_model_grads G;
    G.embed_w = g[0]; G.embed_b = g[1]; G.layers = glayers; G.final_w = g[2 + 16 * L]; G.final_b = g[3 + 16 * L];
    vs_model_desc desc = {D, H, L, DIN, 0, 1};
    vs_weights *w = NULL;
    CHECK(vs_weights_pack(&desc, &P, NULL, &w));

    void *state = NULL, *ws = NULL;
    float *out = NULL, *scale = NULL;
    const size_t nstate = vs_adam_state_bytes(w), nws = vs_grad_norm_workspace_bytes(table, NT);
    if (!nstate || !nws || nws % 256) FAIL("state %zu / workspace %zu bytes", nstate, nws);
    if (hipMalloc(&state, nstate) != hipSuccess || hipMalloc(&ws, nws) != hipSuccess || hipMalloc((void **)&out, 8 * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&scale, sizeof(float)) != hipSuccess) FAIL("hipMalloc");
    const float scalef = 1024.0f;
    hipMemcpy(scale, &scalef, 4, hipMemcpyHostToDevice);
    CHECK(vs_adam_state_init(w, state, NULL));

    vs_adam_cfg cfg = {1e-3, 0.9, 0.999, 1e-8, 1e-5, 0, 0};
    CHECK(vs_grad_norm(w, &G, VS_GRAD_NORM_L2, 1.0, scale, out, ws, nws, NULL));
    CHECK(vs_adam_step(w, &P, &G, state, &cfg, out + 2, NULL, NULL));           /* the clipped step */
    CHECK(vs_grad_norm(w, &G, VS_GRAD_NORM_L2, 1e6, scale, out + 4, ws, nws, NULL));
    if (hipDeviceSynchronize() != hipSuccess) FAIL("hipDeviceSynchronize");
    float r[8], probe = 0.0f, g0 = 0.0f;
    hipMemcpy(r, out, sizeof r, hipMemcpyDeviceToHost);
    hipMemcpy(&probe, p[0] + PROBE, 4, hipMemcpyDeviceToHost);
    hipMemcpy(&g0, g[0], 4, hipMemcpyDeviceToHost);
    if (!(r[0] > 1.0f) || !(r[1] < 1.0f) || r[3] != 0.0f) FAIL("norm %g coef %g: expected a clipped step", r[0], r[1]);
    if (r[4] != r[0] || r[5] != 1.0f || bits(r[6]) != bits(scalef)) FAIL("unclipped: norm %g coef %g divisor %g", r[4], r[5], r[6]);
    if (bits(g0) != bits(hval(100u, 0u) * 16.0f)) FAIL("the gradients were rewritten");
    /* error paths */
    if (vs_grad_norm(w, &G, VS_GRAD_NORM_L2, 0.0, scale, out, ws, nws, NULL) != VS_ERR_INVALID) FAIL("max_norm = 0 accepted");
    if (vs_grad_norm(w, &G, 7, 1.0, scale, out, ws, nws, NULL) != VS_ERR_INVALID) FAIL("kind = 7 accepted");
    if (vs_grad_norm(w, &G, VS_GRAD_NORM_L2, 1.0, scale, out, ws, 8, NULL) != VS_ERR_WORKSPACE) FAIL("a short workspace accepted");
    vs_weights_free(w);
    printf("OK norm %.6f coef %.6f\n", r[0], r[1]);
    printf("%08x\n%08x\n%08x\n%08x\n%08x\n%08x\n%08x\n", bits(r[0]), bits(r[1]), bits(r[2]), bits(probe), bits(r[5]), bits(r[6]), bits(g0));
    return 0;
}
