// vs_optim.hip — the parameter update of the training step (include/vs_optim.h): a multi-tensor Adam kernel for gfx950
// and the C entries over it.
//
// One launch processes a table of up to VS_ADAM_MAX_TENSORS tensors, passed BY VALUE as the kernel's argument: the
// gradient pointers change on every step (the backward allocates a fresh arena) and the launch itself carries them to the
// device - no table upload, no blocking copy, no allocation.  A block owns one CHUNK of one tensor (binary search of its
// block index in the table's chunk prefix).  The kernel is elementwise and HBM-bound: 16-byte accesses, 16 floats per
// thread in flight, 28 bytes moved per element (32 with the mirror).
//
// found_inf / grad_scale are read on the device by every block (uniform loads); a skipped step returns before any store.
// The step count t is read by every block of a tensor and advanced by ONE writer: the block that finishes last in the
// launch (an agent-scope counter of blocks in `sync_word`, which that block also returns to zero).  Every other block
// has read t before it counted itself, so there is no in-launch race and no second launch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "vs_optim.h"
#include "vs_weights_impl.h"

namespace {

constexpr int NT = 256;                       // threads per block (4 waves)
constexpr int VECS = 4;                       // float4 per thread
constexpr unsigned CHUNK = NT * VECS * 4;     // 4096 elements per block

struct AdamTable {
    float *p[VS_ADAM_MAX_TENSORS];
    const float *g[VS_ADAM_MAX_TENSORS];
    float *m[VS_ADAM_MAX_TENSORS];
    float *v[VS_ADAM_MAX_TENSORS];
    float *mirror[VS_ADAM_MAX_TENSORS];
    float *step[VS_ADAM_MAX_TENSORS];
    unsigned n[VS_ADAM_MAX_TENSORS];
    unsigned chunk0[VS_ADAM_MAX_TENSORS + 1];   // first block of tensor i; chunk0[count] = grid size
    int count;
};

struct AdamHyper {
    double lr, beta1, beta2;
    float w1, beta2f, w2, eps, wd, decay;       // (float)(1 - beta1), (float)beta2, (float)(1 - beta2), ..., (float)(1 - lr wd)
    int decoupled;
};

struct AdamConsts {
    float w1, beta2, w2, eps, wd, decay, step_size, bc2_sqrt, scale;
    bool has_scale, decoupled;
};

__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, const AdamConsts &c) {
    if (c.has_scale) g = g / c.scale;
    if (c.decoupled) p = p * c.decay;
    else if (c.wd != 0.0f) g = g + c.wd * p;
    // torch.lerp(m, g, 1 - beta1): the form that is monotonic for the weight at hand
    m = c.w1 < 0.5f ? m + c.w1 * (g - m) : g - (g - m) * (1.0f - c.w1);
    v = v * c.beta2 + (c.w2 * g) * g;
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    p = p - c.step_size * (m / denom);
}

__device__ __forceinline__ void adam_vec(float4 &P, const float4 &G, float4 &M, float4 &V, const AdamConsts &c) {
    adam_one(P.x, G.x, M.x, V.x, c);
    adam_one(P.y, G.y, M.y, V.y, c);
    adam_one(P.z, G.z, M.z, V.z, c);
    adam_one(P.w, G.w, M.w, V.w, c);
}

template <bool FULL>
__device__ __forceinline__ void adam_chunk_vec(float *p, const float *g, float *m, float *v, float *mirror, unsigned len,
                                               const AdamConsts &c) {
    float4 *p4 = reinterpret_cast<float4 *>(p), *m4 = reinterpret_cast<float4 *>(m), *v4 = reinterpret_cast<float4 *>(v);
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    float4 *x4 = reinterpret_cast<float4 *>(mirror);
    const unsigned nv = len >> 2;
    float4 P[VECS], G[VECS], M[VECS], V[VECS];
#pragma unroll
    for (int k = 0; k < VECS; ++k) {
        const unsigned i = threadIdx.x + k * NT;
        if (FULL || i < nv) { P[k] = p4[i]; G[k] = g4[i]; M[k] = m4[i]; V[k] = v4[i]; }
    }
#pragma unroll
    for (int k = 0; k < VECS; ++k) {
        const unsigned i = threadIdx.x + k * NT;
        if (FULL || i < nv) {
            adam_vec(P[k], G[k], M[k], V[k], c);
            p4[i] = P[k]; m4[i] = M[k]; v4[i] = V[k];
            if (mirror) x4[i] = P[k];
        }
    }
    if (!FULL) {
        const unsigned i = (nv << 2) + threadIdx.x;       // the 0..3 elements behind the last whole vector
        if (threadIdx.x < (len & 3u)) {
            float pp = p[i], mm = m[i], vv = v[i];
            adam_one(pp, g[i], mm, vv, c);
            p[i] = pp; m[i] = mm; v[i] = vv;
            if (mirror) mirror[i] = pp;
        }
    }
}

__global__ __launch_bounds__(NT) void adam_multi_tensor(const AdamTable tab, const AdamHyper hp, const float *grad_scale,
                                                        const float *found_inf, unsigned *sync_word) {
    if (found_inf && *found_inf != 0.0f) return;      // skipped step: nothing is written, the counter is not touched
    const unsigned blk = blockIdx.x;
    int lo = 0, hi = tab.count;                        // chunk0[lo] <= blk < chunk0[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab.chunk0[mid] <= blk) lo = mid; else hi = mid;
    }
    const int ti = lo;
    __shared__ float s_c[2];
    __shared__ int s_last;
    if (threadIdx.x == 0) {
        const double t = (double)(*tab.step[ti] + 1.0f);
        s_c[0] = (float)(hp.lr / (1.0 - pow(hp.beta1, t)));
        s_c[1] = (float)sqrt(1.0 - pow(hp.beta2, t));
    }
    __syncthreads();
    AdamConsts c;
    c.w1 = hp.w1; c.beta2 = hp.beta2f; c.w2 = hp.w2; c.eps = hp.eps; c.wd = hp.wd; c.decay = hp.decay;
    c.step_size = s_c[0]; c.bc2_sqrt = s_c[1];
    c.has_scale = grad_scale != nullptr;
    c.scale = c.has_scale ? *grad_scale : 1.0f;
    c.decoupled = hp.decoupled != 0;

    const size_t base = (size_t)(blk - tab.chunk0[ti]) * CHUNK;
    const unsigned n = tab.n[ti];
    const unsigned len = (n - base) < (size_t)CHUNK ? (unsigned)(n - base) : CHUNK;
    float *p = tab.p[ti] + base, *m = tab.m[ti] + base, *v = tab.v[ti] + base;
    const float *g = tab.g[ti] + base;
    float *mirror = tab.mirror[ti] ? tab.mirror[ti] + base : nullptr;
    const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)mirror;
    if ((bits & 15u) == 0) {
        if (len == CHUNK) adam_chunk_vec<true>(p, g, m, v, mirror, len, c);
        else adam_chunk_vec<false>(p, g, m, v, mirror, len, c);
    } else {
        for (unsigned i = threadIdx.x; i < len; i += NT) {
            float pp = p[i], mm = m[i], vv = v[i];
            adam_one(pp, g[i], mm, vv, c);
            p[i] = pp; m[i] = mm; v[i] = vv;
            if (mirror) mirror[i] = pp;
        }
    }

    // The block that counts itself last advances every step count of the launch.  Nothing is handed from block to block
    // here, so no release fence (on gfx950 that is a write-back of the XCD's L2 per block: it made this kernel 4x slower):
    // the only order needed is "thread 0 of every block has READ its step count before it adds to the counter", and it
    // has - the value went into s_c above.
    if (threadIdx.x == 0)
        s_last = __hip_atomic_fetch_add(sync_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    __syncthreads();
    if (s_last) {
        for (int i = threadIdx.x; i < tab.count; i += NT) *tab.step[i] = *tab.step[i] + 1.0f;
        if (threadIdx.x == 0) *sync_word = 0u;
    }
}

int failf(int code, const char *fmt, ...) {
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return vs_fail_msg(code, buf);
}

int check_cfg(const vs_adam_cfg *cfg) {
    if (!cfg) return failf(VS_ERR_INVALID, "vs_adam_cfg is NULL");
    if (!(cfg->lr >= 0.0) || !isfinite(cfg->lr)) return failf(VS_ERR_INVALID, "adam: lr=%g invalid (>= 0)", cfg->lr);
    if (!(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0)) return failf(VS_ERR_INVALID, "adam: beta1=%g invalid ([0, 1))", cfg->beta1);
    if (!(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0)) return failf(VS_ERR_INVALID, "adam: beta2=%g invalid ([0, 1))", cfg->beta2);
    if (!(cfg->eps >= 0.0) || !isfinite(cfg->eps)) return failf(VS_ERR_INVALID, "adam: eps=%g invalid (>= 0)", cfg->eps);
    if (!(cfg->weight_decay >= 0.0) || !isfinite(cfg->weight_decay))
        return failf(VS_ERR_INVALID, "adam: weight_decay=%g invalid (>= 0)", cfg->weight_decay);
    if (cfg->decoupled != 0 && cfg->decoupled != 1) return failf(VS_ERR_INVALID, "adam: decoupled=%d invalid (0 or 1)", cfg->decoupled);
    return VS_OK;
}

AdamHyper make_hyper(const vs_adam_cfg &cfg) {
    AdamHyper hp;
    hp.lr = cfg.lr; hp.beta1 = cfg.beta1; hp.beta2 = cfg.beta2;
    hp.w1 = (float)(1.0 - cfg.beta1); hp.beta2f = (float)cfg.beta2; hp.w2 = (float)(1.0 - cfg.beta2);
    hp.eps = (float)cfg.eps; hp.wd = (float)cfg.weight_decay; hp.decay = (float)(1.0 - cfg.lr * cfg.weight_decay);
    hp.decoupled = cfg.decoupled;
    return hp;
}

// collects tensors into launches of at most VS_ADAM_MAX_TENSORS
struct Launcher {
    AdamTable tab;
    AdamHyper hp;
    const float *grad_scale, *found_inf;
    unsigned *sync_word;
    hipStream_t st;
    hipError_t err = hipSuccess;

    Launcher(const vs_adam_cfg &cfg, const float *gs, const float *fi, void *sw, void *stream)
        : hp(make_hyper(cfg)), grad_scale(gs), found_inf(fi), sync_word((unsigned *)sw), st((hipStream_t)stream) {
        tab.count = 0;
        tab.chunk0[0] = 0;
    }
    void add(float *p, const float *g, float *m, float *v, float *mirror, float *step, size_t n) {
        if (n == 0) return;
        if (tab.count == VS_ADAM_MAX_TENSORS) flush();
        const int i = tab.count++;
        tab.p[i] = p; tab.g[i] = g; tab.m[i] = m; tab.v[i] = v; tab.mirror[i] = mirror; tab.step[i] = step;
        tab.n[i] = (unsigned)n;
        tab.chunk0[i + 1] = tab.chunk0[i] + (unsigned)((n + CHUNK - 1) / CHUNK);
    }
    void flush() {
        if (tab.count > 0 && err == hipSuccess) {
            hipLaunchKernelGGL(adam_multi_tensor, dim3(tab.chunk0[tab.count]), dim3(NT), 0, st, tab, hp, grad_scale, found_inf,
                               sync_word);
            err = hipGetLastError();
        }
        tab.count = 0;
    }
};

// ---- state of a handle: [sync word | 256 B] [step counts] [m of every tensor] [v of every tensor], 256-byte granules ----
struct HandleTensor { size_t blob_off, n; };

size_t pad64(size_t n) { return (n + 63) / 64 * 64; }

int handle_tensor_count(const vs_weights *w) { return 4 + 16 * w->desc.num_layers; }

// tensor `i` in vs_model_params order (include/vs_optim.h: vs_adam_state_field)
HandleTensor handle_tensor(const vs_weights *w, int i) {
    const size_t d = w->desc.d_model, din = w->desc.in_features, nc = w->desc.num_classes;
    const int L = w->desc.num_layers;
    if (i == 0) return {w->embed_w, d * din};
    if (i == 1) return {w->embed_b, d};
    if (i == 2 + 16 * L) return {w->final_w, nc * d};
    if (i == 3 + 16 * L) return {w->final_b, nc};
    const LayerOff &o = w->layers[(i - 2) / 16];
    switch ((i - 2) % 16) {
        case 0: return {o.wqkv, d * d};
        case 1: return {o.bqkv, d};
        case 2: return {o.wqkv + d * d, d * d};
        case 3: return {o.bqkv + d, d};
        case 4: return {o.wqkv + 2 * d * d, d * d};
        case 5: return {o.bqkv + 2 * d, d};
        case 6: return {o.wo, d * d};
        case 7: return {o.bo, d};
        case 8: return {o.ln1g, d};
        case 9: return {o.ln1b, d};
        case 10: return {o.w1, 4 * d * d};
        case 11: return {o.b1, 4 * d};
        case 12: return {o.w2, 4 * d * d};
        case 13: return {o.b2, d};
        case 14: return {o.ln2g, d};
        default: return {o.ln2b, d};
    }
}

constexpr size_t STATE_HEADER_FLOATS = 64;

size_t state_m_floats(const vs_weights *w) {
    size_t s = 0;
    for (int i = 0, n = handle_tensor_count(w); i < n; ++i) s += pad64(handle_tensor(w, i).n);
    return s;
}

const float *const *layer_field(const vs_layer_params &P, int j) { return &P.wq + j; }
float *const *layer_field(const vs_layer_grads &G, int j) { return &G.wq + j; }

}  // namespace

static_assert(sizeof(vs_layer_params) == 16 * sizeof(void *) && sizeof(vs_layer_grads) == 16 * sizeof(void *),
              "vs_layer_params / vs_layer_grads: 16 pointers in declaration order");
static_assert(sizeof(AdamTable) + sizeof(AdamHyper) + 3 * sizeof(void *) <= 4096, "kernel arguments stay below 4 KiB");

extern "C" {

int vs_adam_step_tensors(const vs_adam_tensor *table, int32_t n_tensors, const vs_adam_cfg *cfg, const float *grad_scale,
                         const float *found_inf, void *sync_word, void *stream) {
    if (n_tensors < 0) return failf(VS_ERR_INVALID, "vs_adam_step_tensors: n_tensors=%d", n_tensors);
    if (n_tensors > 0 && !table) return failf(VS_ERR_INVALID, "vs_adam_step_tensors: table is NULL");
    if (!sync_word) return failf(VS_ERR_INVALID, "vs_adam_step_tensors: sync_word is NULL");
    if (int rc = check_cfg(cfg)) return rc;
    for (int i = 0; i < n_tensors; ++i) {
        const vs_adam_tensor &t = table[i];
        if (t.n == 0) continue;
        if (!t.p || !t.g || !t.m || !t.v || !t.step)
            return failf(VS_ERR_INVALID, "vs_adam_step_tensors: tensor %d has a NULL p / g / m / v / step pointer", i);
        if (t.n >= ((size_t)1 << 32)) return failf(VS_ERR_INVALID, "vs_adam_step_tensors: tensor %d has %zu elements (< 2^32)", i, t.n);
    }
    Launcher ln(*cfg, grad_scale, found_inf, sync_word, stream);
    for (int i = 0; i < n_tensors; ++i) {
        const vs_adam_tensor &t = table[i];
        ln.add(t.p, t.g, t.m, t.v, t.mirror, t.step, t.n);
    }
    ln.flush();
    if (ln.err != hipSuccess) return failf(VS_ERR_HIP, "adam launch failed: %s", hipGetErrorString(ln.err));
    return VS_OK;
}

size_t vs_adam_state_bytes(const vs_weights *w) {
    if (!w) return 0;
    return (STATE_HEADER_FLOATS + pad64((size_t)handle_tensor_count(w)) + 2 * state_m_floats(w)) * sizeof(float);
}

int vs_adam_state_init(const vs_weights *w, void *state, void *stream) {
    if (!w || !state) return failf(VS_ERR_INVALID, "vs_adam_state_init: weights/state is NULL");
    if ((uintptr_t)state & 255u) return failf(VS_ERR_INVALID, "vs_adam_state_init: state must be 256-byte aligned");
    const hipError_t e = hipMemsetAsync(state, 0, vs_adam_state_bytes(w), (hipStream_t)stream);
    if (e != hipSuccess) return failf(VS_ERR_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    return VS_OK;
}

int vs_adam_state_field(const vs_weights *w, int32_t tensor, int32_t which, size_t *offset_bytes, size_t *count) {
    if (!w || !offset_bytes || !count) return failf(VS_ERR_INVALID, "vs_adam_state_field: NULL argument");
    const int nt = handle_tensor_count(w);
    if (tensor < 0 || tensor >= nt) return failf(VS_ERR_INVALID, "vs_adam_state_field: tensor=%d outside [0, %d)", tensor, nt);
    if (which < 0 || which > 2) return failf(VS_ERR_INVALID, "vs_adam_state_field: which=%d (0 m, 1 v, 2 step)", which);
    if (which == 2) {
        *offset_bytes = (STATE_HEADER_FLOATS + (size_t)tensor) * sizeof(float);
        *count = 1;
        return VS_OK;
    }
    size_t off = STATE_HEADER_FLOATS + pad64((size_t)nt) + (which == 1 ? state_m_floats(w) : 0);
    for (int i = 0; i < tensor; ++i) off += pad64(handle_tensor(w, i).n);
    *offset_bytes = off * sizeof(float);
    *count = handle_tensor(w, tensor).n;
    return VS_OK;
}

int vs_adam_step(vs_weights *w, const vs_model_params *params, const vs_model_grads *grads, void *state,
                 const vs_adam_cfg *cfg, const float *grad_scale, const float *found_inf, void *stream) {
    if (!w || !grads || !state) return failf(VS_ERR_INVALID, "vs_adam_step: weights/grads/state is NULL");
    if ((uintptr_t)state & 255u) return failf(VS_ERR_INVALID, "vs_adam_step: state must be 256-byte aligned");
    if (int rc = check_cfg(cfg)) return rc;
    if (w->embedded())
        return failf(VS_ERR_INVALID, "vs_adam_step: the handle embeds a d_model=%d model in d_model=%d; use vs_adam_step_tensors on the "
                                     "caller's tensors and vs_weights_update", w->dn(), w->desc.d_model);
    const int L = w->desc.num_layers, nt = handle_tensor_count(w);
    if (L > 0 && (!grads->layers || (params && !params->layers))) return failf(VS_ERR_INVALID, "vs_adam_step: layers is NULL");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != w->device)
        return failf(VS_ERR_INVALID, "vs_adam_step on device %d, handle was packed on device %d", dev, w->device);
    auto grad_of = [&](int i) -> const float * {
        if (i == 0) return grads->embed_w;
        if (i == 1) return grads->embed_b;
        if (i == 2 + 16 * L) return grads->final_w;
        if (i == 3 + 16 * L) return grads->final_b;
        return *layer_field(grads->layers[(i - 2) / 16], (i - 2) % 16);
    };
    auto param_of = [&](int i) -> const float * {
        if (i == 0) return params->embed_w;
        if (i == 1) return params->embed_b;
        if (i == 2 + 16 * L) return params->final_w;
        if (i == 3 + 16 * L) return params->final_b;
        return *layer_field(params->layers[(i - 2) / 16], (i - 2) % 16);
    };
    if (params)
        for (int i = 0; i < nt; ++i)
            if (grad_of(i) && !param_of(i)) return failf(VS_ERR_INVALID, "vs_adam_step: tensor %d has a gradient but a NULL parameter pointer", i);
    float *sf = (float *)state;
    float *steps = sf + STATE_HEADER_FLOATS;
    float *m = steps + pad64((size_t)nt);
    float *v = m + state_m_floats(w);
    vsw_order(w, stream);       // images still being read / built on another stream
    Launcher ln(*cfg, grad_scale, found_inf, state, stream);
    for (int i = 0; i < nt; ++i) {
        const HandleTensor t = handle_tensor(w, i);
        if (const float *g = grad_of(i)) {
            float *slot = w->blob + t.blob_off;
            if (params) ln.add(const_cast<float *>(param_of(i)), g, m, v, slot, steps + i, t.n);
            else ln.add(slot, g, m, v, nullptr, steps + i, t.n);
        }
        m += pad64(t.n);
        v += pad64(t.n);
    }
    ln.flush();
    ++w->version;        // as vs_weights_update: every image family and the transposes are rebuilt on their next use
    vsw_mark(w, stream);
    if (ln.err != hipSuccess) return failf(VS_ERR_HIP, "adam launch failed: %s", hipGetErrorString(ln.err));
    return VS_OK;
}

}  // extern "C"
