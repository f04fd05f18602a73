/* optim_demo.c — a training LOOP from plain C: no Python, no torch.  Build like train_demo.c (tests/test_cabi_optim.py
 * does it and runs it on the GPU box).
 * Random small model (d 128, 2 heads of 64, 2 layers), a padded batch with a key mask and a smooth target, then STEPS times:
 *   vs_train_forward -> vs_mse_mask_loss_forward / _backward -> vs_train_backward -> vs_adam_step(params = NULL)
 * The packed copy inside the handle is the only copy of the parameters: the optimizer updates it in place and no
 * vs_weights_update is ever called.  A device-side loss scale (2^10) and overflow flag (0) go with every step, as a
 * GradScaler would pass them; one extra step with the flag raised must change nothing.
 * Prints "OK", then every loss as its bit pattern (two runs print identical lines). */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vs_optim.h"

static uint32_t rng_state = 97531u;
static float rnd(void) { rng_state = rng_state * 1664525u + 1013904223u; return (float)(rng_state >> 8) / 8388608.0f - 1.0f; }
static float *dev_random(size_t n, float scale, float offset) {
    float *h = (float *)malloc(n * sizeof(float)), *d = NULL;
    for (size_t i = 0; i < n; ++i) h[i] = rnd() * scale + offset;
    if (hipMalloc((void **)&d, n * sizeof(float)) != hipSuccess) exit(2);
    hipMemcpy(d, h, n * sizeof(float), hipMemcpyHostToDevice);
    free(h);
    return d;
}
static float *dev_alloc(size_t n) { float *d = NULL; if (hipMalloc((void **)&d, n * sizeof(float)) != hipSuccess) exit(2); return d; }
static float host_scalar(const float *d) { float h; hipDeviceSynchronize(); hipMemcpy(&h, d, 4, hipMemcpyDeviceToHost); return h; }
#define CHECK(call) do { int rc_ = (call); if (rc_ != VS_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, vs_last_error()); return 1; } } while (0)
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

enum { D = 128, H = 2, L = 2, DIN = 1024, MAXLEN = 2000, B = 2, T = 90, STEPS = 24 };

int main(void) {
    const int lengths[B] = {90, 57};
    vs_layer_params layers[L];
    vs_layer_grads glayers[L];
    for (int l = 0; l < L; ++l) {
        const float s = 1.0f / 11.0f;
        layers[l].wq = dev_random(D * D, s, 0); layers[l].bq = dev_random(D, 0.1f, 0);
        layers[l].wk = dev_random(D * D, s, 0); layers[l].bk = dev_random(D, 0.1f, 0);
        layers[l].wv = dev_random(D * D, s, 0); layers[l].bv = dev_random(D, 0.1f, 0);
        layers[l].wo = dev_random(D * D, s, 0); layers[l].bo = dev_random(D, 0.1f, 0);
        layers[l].ln1_g = dev_random(D, 0.1f, 1.0f); layers[l].ln1_b = dev_random(D, 0.1f, 0);
        layers[l].w1 = dev_random(4 * D * D, s, 0); layers[l].b1 = dev_random(4 * D, 0.1f, 0);
        layers[l].w2 = dev_random(4 * D * D, s / 2, 0); layers[l].b2 = dev_random(D, 0.1f, 0);
        layers[l].ln2_g = dev_random(D, 0.1f, 1.0f); layers[l].ln2_b = dev_random(D, 0.1f, 0);
        glayers[l].wq = dev_alloc(D * D); glayers[l].bq = dev_alloc(D); glayers[l].wk = dev_alloc(D * D); glayers[l].bk = dev_alloc(D);
        glayers[l].wv = dev_alloc(D * D); glayers[l].bv = dev_alloc(D); glayers[l].wo = dev_alloc(D * D); glayers[l].bo = dev_alloc(D);
        glayers[l].ln1_g = dev_alloc(D); glayers[l].ln1_b = dev_alloc(D); glayers[l].w1 = dev_alloc(4 * D * D); glayers[l].b1 = dev_alloc(4 * D);
        glayers[l].w2 = dev_alloc(4 * D * D); glayers[l].b2 = dev_alloc(D); glayers[l].ln2_g = dev_alloc(D); glayers[l].ln2_b = dev_alloc(D);
    }
    vs_model_params P;
    P.embed_w = dev_random((size_t)D * DIN, 1.0f / 32.0f, 0); P.embed_b = dev_random(D, 0.1f, 0);
    P.pos_embedding = dev_random((size_t)MAXLEN * D, 1.0f, 0);
    P.layers = layers;
    P.final_w = dev_random(D, 1.0f / 11.0f, 0); P.final_b = dev_random(1, 0.1f, 0);
    vs_model_grads G;
    G.embed_w = dev_alloc((size_t)D * DIN); G.embed_b = dev_alloc(D); G.layers = glayers; G.final_w = dev_alloc(D); G.final_b = dev_alloc(1);
    vs_model_desc desc = {D, H, L, DIN, MAXLEN, 1};
    vs_weights *w = NULL;
    CHECK(vs_weights_pack(&desc, &P, NULL, &w));      /* from here on the handle owns the only copy that is trained */

    float *hx = (float *)malloc((size_t)B * T * DIN * 4), htgt[B * T];
    uint8_t hmask[B * T];
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < T; ++t) {
            float acc = 0.0f;
            hmask[b * T + t] = t >= lengths[b];
            for (int c = 0; c < DIN; ++c) {
                const float xv = t < lengths[b] ? fabsf(rnd()) * 0.5f : 1000.0f;
                hx[((size_t)b * T + t) * DIN + c] = xv;
                if (c < 16) acc += c < 8 ? xv : -xv;
            }
            htgt[b * T + t] = 1.0f / (1.0f + expf(-acc));        /* a smooth function of two feature directions */
        }
    float *x = dev_alloc((size_t)B * T * DIN), *tgt = dev_alloc(B * T), *scores = dev_alloc(B * T);
    float *dsc = dev_alloc(B * T), *loss = dev_alloc(1), *scratch = dev_alloc(256), *scale = dev_alloc(1), *found_inf = dev_alloc(1);
    uint8_t *mask = NULL; hipMalloc((void **)&mask, B * T);
    hipMemcpy(x, hx, (size_t)B * T * DIN * 4, hipMemcpyHostToDevice); hipMemcpy(mask, hmask, B * T, hipMemcpyHostToDevice);
    hipMemcpy(tgt, htgt, sizeof htgt, hipMemcpyHostToDevice);
    const float scalef = 1024.0f, zerof = 0.0f, onef = 1.0f;
    hipMemcpy(scale, &scalef, 4, hipMemcpyHostToDevice); hipMemcpy(found_inf, &zerof, 4, hipMemcpyHostToDevice);
    void *saved = NULL, *ws = NULL, *state = NULL;
    const size_t nsaved = vs_train_saved_bytes(w, B, T), nws = vs_train_workspace_bytes(w, B, T), nstate = vs_adam_state_bytes(w);
    hipMalloc(&saved, nsaved); hipMalloc(&ws, nws); hipMalloc(&state, nstate);
    if (!nstate) FAIL("vs_adam_state_bytes is 0");
    CHECK(vs_train_prepare(w, NULL));
    CHECK(vs_adam_state_init(w, state, NULL));

    vs_adam_cfg cfg = {1e-3, 0.9, 0.999, 1e-8, 1e-5, 0, 0};
    float losses[STEPS + 2];
    for (int it = 0; it < STEPS + 2; ++it) {
        CHECK(vs_train_forward(w, x, mask, B, T, NULL, scores, NULL, saved, nsaved, ws, nws, NULL));
        CHECK(vs_mse_mask_loss_forward(scores, tgt, mask, B * T, 1, scratch, loss, NULL));
        losses[it] = host_scalar(loss);
        if (!isfinite(losses[it])) FAIL("loss %d is not finite", it);
        if (it == STEPS + 1) break;                                    /* the last pass only measures */
        CHECK(vs_mse_mask_loss_backward(scores, tgt, mask, scale, B * T, 1, dsc, NULL));     /* d_loss = the loss scale */
        CHECK(vs_train_backward(w, x, mask, B, T, NULL, dsc, NULL, saved, nsaved, &G, NULL, ws, nws, NULL));
        if (it == STEPS) hipMemcpy(found_inf, &onef, 4, hipMemcpyHostToDevice);              /* an "overflow": this step is skipped */
        cfg.lr = it < 4 ? 2.5e-4 * (it + 1) : 1e-3;                    /* a warm-up written into the struct, as a scheduler would */
        CHECK(vs_adam_step(w, NULL, &G, state, &cfg, scale, found_inf, NULL));
    }
    if (!(losses[STEPS] < losses[0])) FAIL("loss did not fall: %g -> %g", losses[0], losses[STEPS]);
    if (memcmp(&losses[STEPS], &losses[STEPS + 1], 4)) FAIL("a skipped step changed the model: %g -> %g", losses[STEPS], losses[STEPS + 1]);
    float steps_done = 0.0f;
    size_t off = 0, cnt = 0;
    CHECK(vs_adam_state_field(w, 0, 2, &off, &cnt));
    hipMemcpy(&steps_done, (char *)state + off, 4, hipMemcpyDeviceToHost);
    if (steps_done != (float)STEPS) FAIL("step count %g, expected %d", steps_done, STEPS);
    /* error paths */
    cfg.beta1 = 1.0;
    if (vs_adam_step(w, NULL, &G, state, &cfg, NULL, NULL, NULL) != VS_ERR_INVALID) FAIL("beta1 = 1 accepted");
    vs_weights_free(w);
    printf("OK loss %.6f -> %.6f in %d Adam steps\n", losses[0], losses[STEPS], STEPS);
    for (int it = 0; it <= STEPS + 1; ++it) { uint32_t u; memcpy(&u, &losses[it], 4); printf("%08x\n", u); }
    return 0;
}
