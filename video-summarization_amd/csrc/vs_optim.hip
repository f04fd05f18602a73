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
//
// Clipping the global gradient norm (further down): grad_sumsq_multi_tensor + grad_norm_finalize measure the norm of all
// gradients and write grad_scale / clip_coef into a device scalar that adam_multi_tensor takes as its grad_scale - the
// update kernel itself is unchanged; grad_scale_multi_tensor scales gradients in place for a loop with another optimizer.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "vs_error.h"
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

// ---- the global gradient norm (clipping) ---------------------------------------------------------------------------
// Same table-in-the-launch form and the same chunking as the Adam kernel.  A block reduces ONE chunk to ONE double and
// stores it at the chunk's GLOBAL index in the caller's workspace; grad_norm_finalize, a second small launch, reduces those
// and writes the four scalars of include/vs_optim.h.  Nothing is handed from block to block inside a launch (that would
// need the release fence the note above prices), and because a partial depends on its chunk alone and the finalize order on
// the chunk index alone, the norm does not depend on how the tensors were grouped into launches.
//
// The squares are accumulated in double from the element up: an fp32 x fp32 product is exact in double, so the only error
// is the sum's (n 2^-53).  The element -> thread assignment is the same on the 16-byte path and on the element path, so the
// bits do not depend on a tensor's alignment either.  fp64 FMA runs at half the fp32 VALU rate; at 4 bytes and one
// multiply-add per element the kernel stays far below it.
struct GradTable {
    float *g[VS_ADAM_MAX_TENSORS];
    unsigned n[VS_ADAM_MAX_TENSORS];
    unsigned chunk0[VS_ADAM_MAX_TENSORS + 1];   // first block of tensor i; chunk0[count] = grid size
    int count;
    unsigned first;                             // global index of this launch's first chunk
};

__device__ __forceinline__ int table_find(const unsigned *chunk0, int count, unsigned blk) {
    int lo = 0, hi = count;                     // chunk0[lo] <= blk < chunk0[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk0[mid] <= blk) lo = mid; else hi = mid;
    }
    return lo;
}

// L2: a + b.  Max: the larger, a NaN wins (torch's norm propagates it; fmax would drop it).
template <int KIND>
__device__ __forceinline__ double norm_combine(double a, double b) {
    if (KIND == VS_GRAD_NORM_L2) return a + b;
    return a != a ? a : (b != b ? b : (a > b ? a : b));
}

template <int KIND>
__device__ __forceinline__ void norm_take(double &acc, float x) {
    const double d = (double)x;
    if (KIND == VS_GRAD_NORM_L2) acc = fma(d, d, acc);      // d * d is exact: the same bits with or without contraction
    else acc = norm_combine<KIND>(acc, fabs(d));
}

// lane, wave, block: a fixed order.  The result is valid in thread 0.
template <int KIND>
__device__ __forceinline__ double norm_block_reduce(double v, double *s_w) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = norm_combine<KIND>(v, __shfl_down(v, off, 64));
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        v = s_w[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) v = norm_combine<KIND>(v, s_w[w]);
    }
    return v;
}

template <int KIND>
__global__ __launch_bounds__(NT) void grad_sumsq_multi_tensor(const GradTable tab, double *partials) {
    const unsigned blk = blockIdx.x;
    const int ti = table_find(tab.chunk0, tab.count, blk);
    const size_t base = (size_t)(blk - tab.chunk0[ti]) * CHUNK;
    const unsigned n = tab.n[ti];
    const unsigned len = (n - base) < (size_t)CHUNK ? (unsigned)(n - base) : CHUNK;
    const float *g = tab.g[ti] + base;
    const unsigned nv = len >> 2;
    const bool vec = ((uintptr_t)g & 15u) == 0;
    float4 G[VECS];
#pragma unroll
    for (int k = 0; k < VECS; ++k) {
        const unsigned i = threadIdx.x + k * NT;
        G[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);         // adds +0 / is never the larger: no effect on either norm
        if (i < nv) {
            if (vec) G[k] = reinterpret_cast<const float4 *>(g)[i];
            else G[k] = make_float4(g[4 * i], g[4 * i + 1], g[4 * i + 2], g[4 * i + 3]);
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < VECS; ++k) {
        norm_take<KIND>(acc, G[k].x);
        norm_take<KIND>(acc, G[k].y);
        norm_take<KIND>(acc, G[k].z);
        norm_take<KIND>(acc, G[k].w);
    }
    if (threadIdx.x < (len & 3u)) norm_take<KIND>(acc, g[(nv << 2) + threadIdx.x]);   // the 0..3 elements behind the last vector
    __shared__ double s_w[NT / 64];
    acc = norm_block_reduce<KIND>(acc, s_w);
    if (threadIdx.x == 0) partials[(size_t)tab.first + blk] = acc;
}

template <int KIND>
__global__ __launch_bounds__(NT) void grad_norm_finalize(const double *partials, unsigned count, double max_norm,
                                                         const float *grad_scale, float *out) {
    double acc = 0.0;
    for (unsigned i = threadIdx.x; i < count; i += NT) acc = norm_combine<KIND>(acc, partials[i]);
    __shared__ double s_w[NT / 64];
    acc = norm_block_reduce<KIND>(acc, s_w);
    if (threadIdx.x == 0) {
        const float scale_f = grad_scale ? *grad_scale : 1.0f;
        const double scale = (double)scale_f;
        const double norm = (KIND == VS_GRAD_NORM_L2 ? sqrt(acc) : acc) / scale;
        double coef = max_norm / (norm + 1e-6);             // torch.nn.utils.clip_grad_norm_'s formula ...
        coef = coef < 1.0 ? coef : (coef != coef ? coef : 1.0);        // ... and its clamp(max = 1), which keeps a NaN
        const float coef_f = (float)coef;
        out[0] = (float)norm;
        out[1] = coef_f;
        out[2] = coef_f == 1.0f ? scale_f : (float)(scale / coef);     // the divisor of the Adam kernel: one rounding
        out[3] = 0.0f;
    }
}

__global__ __launch_bounds__(NT) void grad_scale_multi_tensor(const GradTable tab, const float *coef) {
    const float c = *coef;
    if (c == 1.0f) return;                      // within the threshold: the gradients keep their bits, nothing is written
    const unsigned blk = blockIdx.x;
    const int ti = table_find(tab.chunk0, tab.count, blk);
    const size_t base = (size_t)(blk - tab.chunk0[ti]) * CHUNK;
    const unsigned n = tab.n[ti];
    const unsigned len = (n - base) < (size_t)CHUNK ? (unsigned)(n - base) : CHUNK;
    float *g = tab.g[ti] + base;
    if (((uintptr_t)g & 15u) == 0) {
        float4 *g4 = reinterpret_cast<float4 *>(g);
        const unsigned nv = len >> 2;
        float4 G[VECS];
#pragma unroll
        for (int k = 0; k < VECS; ++k) {
            const unsigned i = threadIdx.x + k * NT;
            if (i < nv) G[k] = g4[i];
        }
#pragma unroll
        for (int k = 0; k < VECS; ++k) {
            const unsigned i = threadIdx.x + k * NT;
            if (i < nv) g4[i] = make_float4(G[k].x * c, G[k].y * c, G[k].z * c, G[k].w * c);
        }
        const unsigned i = (nv << 2) + threadIdx.x;
        if (threadIdx.x < (len & 3u)) g[i] = g[i] * c;
    } else {
        for (unsigned i = threadIdx.x; i < len; i += NT) g[i] = g[i] * c;
    }
}

int check_cfg(const vs_adam_cfg *cfg) {
    if (!cfg) return vs_failf(VS_ERR_INVALID, "vs_adam_cfg is NULL");
    if (!(cfg->lr >= 0.0) || !isfinite(cfg->lr)) return vs_failf(VS_ERR_INVALID, "adam: lr=%g invalid (>= 0)", cfg->lr);
    if (!(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0)) return vs_failf(VS_ERR_INVALID, "adam: beta1=%g invalid ([0, 1))", cfg->beta1);
    if (!(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0)) return vs_failf(VS_ERR_INVALID, "adam: beta2=%g invalid ([0, 1))", cfg->beta2);
    if (!(cfg->eps >= 0.0) || !isfinite(cfg->eps)) return vs_failf(VS_ERR_INVALID, "adam: eps=%g invalid (>= 0)", cfg->eps);
    if (!(cfg->weight_decay >= 0.0) || !isfinite(cfg->weight_decay))
        return vs_failf(VS_ERR_INVALID, "adam: weight_decay=%g invalid (>= 0)", cfg->weight_decay);
    if (cfg->decoupled != 0 && cfg->decoupled != 1) return vs_failf(VS_ERR_INVALID, "adam: decoupled=%d invalid (0 or 1)", cfg->decoupled);
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

// the same for the gradient-only kernels: norm partials (partials != NULL) or the in-place scale (coef != NULL)
struct GradLauncher {
    GradTable tab;
    int kind;
    double *partials;
    const float *coef;
    hipStream_t st;
    hipError_t err = hipSuccess;

    GradLauncher(int kind_, double *partials_, const float *coef_, void *stream)
        : kind(kind_), partials(partials_), coef(coef_), st((hipStream_t)stream) {
        tab.count = 0;
        tab.chunk0[0] = 0;
        tab.first = 0;
    }
    void add(float *g, size_t n) {
        if (!g || n == 0) return;
        if (tab.count == VS_ADAM_MAX_TENSORS) flush();
        const int i = tab.count++;
        tab.g[i] = g;
        tab.n[i] = (unsigned)n;
        tab.chunk0[i + 1] = tab.chunk0[i] + (unsigned)((n + CHUNK - 1) / CHUNK);
    }
    void flush() {
        if (tab.count > 0 && err == hipSuccess) {
            const dim3 grid(tab.chunk0[tab.count]), block(NT);
            if (coef) hipLaunchKernelGGL(grad_scale_multi_tensor, grid, block, 0, st, tab, coef);
            else if (kind == VS_GRAD_NORM_L2) hipLaunchKernelGGL(grad_sumsq_multi_tensor<VS_GRAD_NORM_L2>, grid, block, 0, st, tab, partials);
            else hipLaunchKernelGGL(grad_sumsq_multi_tensor<VS_GRAD_NORM_MAX>, grid, block, 0, st, tab, partials);
            err = hipGetLastError();
        }
        tab.first += tab.chunk0[tab.count];
        tab.count = 0;
    }
    unsigned chunks() const { return tab.first + tab.chunk0[tab.count]; }
};

constexpr size_t GRAD_MAX_CHUNKS = (size_t)1 << 31;

size_t grad_ws_bytes(size_t chunks) { return ((chunks > 0 ? chunks : 1) * sizeof(double) + 255) / 256 * 256; }

// chunks of a table; (size_t)-1 when an entry is invalid
size_t grad_table_chunks(const vs_grad_tensor *table, int32_t n_tensors, const char *who, bool report) {
    size_t chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const vs_grad_tensor &t = table[i];
        if (!t.g || t.n == 0) continue;
        if (t.n >= ((size_t)1 << 32)) {
            if (report) vs_failf(VS_ERR_INVALID, "%s: tensor %d has %zu elements (< 2^32)", who, i, t.n);
            return (size_t)-1;
        }
        chunks += (t.n + CHUNK - 1) / CHUNK;
    }
    if (chunks >= GRAD_MAX_CHUNKS) {
        if (report) vs_failf(VS_ERR_INVALID, "%s: %zu chunks of %u elements (< 2^31)", who, chunks, CHUNK);
        return (size_t)-1;
    }
    return chunks;
}

int check_norm_args(const char *who, int32_t kind, double max_norm, const float *out, const void *workspace) {
    if (!out) return vs_failf(VS_ERR_INVALID, "%s: out is NULL", who);
    if (!workspace) return vs_failf(VS_ERR_INVALID, "%s: workspace is NULL", who);
    if ((uintptr_t)workspace & 7u) return vs_failf(VS_ERR_INVALID, "%s: workspace must be 8-byte aligned", who);
    if (kind != VS_GRAD_NORM_L2 && kind != VS_GRAD_NORM_MAX) return vs_failf(VS_ERR_INVALID, "%s: kind=%d (0 L2, 1 max)", who, kind);
    if (!(max_norm > 0.0)) return vs_failf(VS_ERR_INVALID, "%s: max_norm=%g invalid (> 0; +inf measures only)", who, max_norm);
    return VS_OK;
}

int norm_finish(GradLauncher &ln, int32_t kind, double max_norm, const float *grad_scale, float *out) {
    ln.flush();
    if (ln.err == hipSuccess) {
        if (kind == VS_GRAD_NORM_L2)
            hipLaunchKernelGGL(grad_norm_finalize<VS_GRAD_NORM_L2>, dim3(1), dim3(NT), 0, ln.st, ln.partials, ln.chunks(), max_norm, grad_scale, out);
        else
            hipLaunchKernelGGL(grad_norm_finalize<VS_GRAD_NORM_MAX>, dim3(1), dim3(NT), 0, ln.st, ln.partials, ln.chunks(), max_norm, grad_scale, out);
        ln.err = hipGetLastError();
    }
    if (ln.err != hipSuccess) return vs_failf(VS_ERR_HIP, "grad norm launch failed: %s", hipGetErrorString(ln.err));
    return VS_OK;
}

// ---- state of a handle: [sync word | 256 B] [step counts] [m of every tensor] [v of every tensor], 256-byte granules ----
size_t pad64(size_t n) { return (n + 63) / 64 * 64; }

// the handle's tensors in vs_model_params order (include/vs_optim.h: vs_adam_state_field): the layout's tensor table
int handle_tensor_count(const vs_weights *w) { return (int)w->tensors.size(); }
const VsTensorAt &handle_tensor(const vs_weights *w, int i) { return w->tensors[i]; }

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
    if (n_tensors < 0) return vs_failf(VS_ERR_INVALID, "vs_adam_step_tensors: n_tensors=%d", n_tensors);
    if (n_tensors > 0 && !table) return vs_failf(VS_ERR_INVALID, "vs_adam_step_tensors: table is NULL");
    if (!sync_word) return vs_failf(VS_ERR_INVALID, "vs_adam_step_tensors: sync_word is NULL");
    if (int rc = check_cfg(cfg)) return rc;
    for (int i = 0; i < n_tensors; ++i) {
        const vs_adam_tensor &t = table[i];
        if (t.n == 0) continue;
        if (!t.p || !t.g || !t.m || !t.v || !t.step)
            return vs_failf(VS_ERR_INVALID, "vs_adam_step_tensors: tensor %d has a NULL p / g / m / v / step pointer", i);
        if (t.n >= ((size_t)1 << 32)) return vs_failf(VS_ERR_INVALID, "vs_adam_step_tensors: tensor %d has %zu elements (< 2^32)", i, t.n);
    }
    Launcher ln(*cfg, grad_scale, found_inf, sync_word, stream);
    for (int i = 0; i < n_tensors; ++i) {
        const vs_adam_tensor &t = table[i];
        ln.add(t.p, t.g, t.m, t.v, t.mirror, t.step, t.n);
    }
    ln.flush();
    if (ln.err != hipSuccess) return vs_failf(VS_ERR_HIP, "adam launch failed: %s", hipGetErrorString(ln.err));
    return VS_OK;
}

size_t vs_adam_state_bytes(const vs_weights *w) {
    if (!w) return 0;
    return (STATE_HEADER_FLOATS + pad64((size_t)handle_tensor_count(w)) + 2 * state_m_floats(w)) * sizeof(float);
}

int vs_adam_state_init(const vs_weights *w, void *state, void *stream) {
    if (!w || !state) return vs_failf(VS_ERR_INVALID, "vs_adam_state_init: weights/state is NULL");
    if ((uintptr_t)state & 255u) return vs_failf(VS_ERR_INVALID, "vs_adam_state_init: state must be 256-byte aligned");
    const hipError_t e = hipMemsetAsync(state, 0, vs_adam_state_bytes(w), (hipStream_t)stream);
    if (e != hipSuccess) return vs_failf(VS_ERR_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    return VS_OK;
}

int vs_adam_state_field(const vs_weights *w, int32_t tensor, int32_t which, size_t *offset_bytes, size_t *count) {
    if (!w || !offset_bytes || !count) return vs_failf(VS_ERR_INVALID, "vs_adam_state_field: NULL argument");
    const int nt = handle_tensor_count(w);
    if (tensor < 0 || tensor >= nt) return vs_failf(VS_ERR_INVALID, "vs_adam_state_field: tensor=%d outside [0, %d)", tensor, nt);
    if (which < 0 || which > 2) return vs_failf(VS_ERR_INVALID, "vs_adam_state_field: which=%d (0 m, 1 v, 2 step)", which);
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
    if (!w || !grads || !state) return vs_failf(VS_ERR_INVALID, "vs_adam_step: weights/grads/state is NULL");
    if ((uintptr_t)state & 255u) return vs_failf(VS_ERR_INVALID, "vs_adam_step: state must be 256-byte aligned");
    if (int rc = check_cfg(cfg)) return rc;
    if (w->embedded())
        return vs_failf(VS_ERR_INVALID, "vs_adam_step: the handle embeds a d_model=%d model in d_model=%d; use vs_adam_step_tensors on the "
                                     "caller's tensors and vs_weights_update", w->dn(), w->desc.d_model);
    const int L = w->desc.num_layers, nt = handle_tensor_count(w);
    if (L > 0 && (!grads->layers || (params && !params->layers))) return vs_failf(VS_ERR_INVALID, "vs_adam_step: layers is NULL");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != w->device)
        return vs_failf(VS_ERR_INVALID, "vs_adam_step on device %d, handle was packed on device %d", dev, w->device);
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
            if (grad_of(i) && !param_of(i)) return vs_failf(VS_ERR_INVALID, "vs_adam_step: tensor %d has a gradient but a NULL parameter pointer", i);
    float *sf = (float *)state;
    float *steps = sf + STATE_HEADER_FLOATS;
    float *m = steps + pad64((size_t)nt);
    float *v = m + state_m_floats(w);
    vsw_order(w, stream);       // images still being read / built on another stream
    Launcher ln(*cfg, grad_scale, found_inf, state, stream);
    for (int i = 0; i < nt; ++i) {
        const VsTensorAt &t = handle_tensor(w, i);
        if (const float *g = grad_of(i)) {
            float *slot = w->blob + t.off;
            if (params) ln.add(const_cast<float *>(param_of(i)), g, m, v, slot, steps + i, t.n);
            else ln.add(slot, g, m, v, nullptr, steps + i, t.n);
        }
        m += pad64(t.n);
        v += pad64(t.n);
    }
    ln.flush();
    ++w->version;        // as vs_weights_update: every image family and the transposes are rebuilt on their next use
    vsw_mark(w, stream);
    if (ln.err != hipSuccess) return vs_failf(VS_ERR_HIP, "adam launch failed: %s", hipGetErrorString(ln.err));
    return VS_OK;
}

size_t vs_grad_norm_workspace_bytes(const vs_grad_tensor *table, int32_t n_tensors) {
    if (n_tensors < 0 || !table) return 0;
    const size_t chunks = grad_table_chunks(table, n_tensors, "vs_grad_norm_workspace_bytes", false);
    return chunks == (size_t)-1 ? 0 : grad_ws_bytes(chunks);
}

int vs_grad_norm_tensors(const vs_grad_tensor *table, int32_t n_tensors, int32_t kind, double max_norm,
                         const float *grad_scale, float *out, void *workspace, size_t workspace_bytes, void *stream) {
    if (n_tensors < 0) return vs_failf(VS_ERR_INVALID, "vs_grad_norm_tensors: n_tensors=%d", n_tensors);
    if (!table) return vs_failf(VS_ERR_INVALID, "vs_grad_norm_tensors: table is NULL");
    if (int rc = check_norm_args("vs_grad_norm_tensors", kind, max_norm, out, workspace)) return rc;
    const size_t chunks = grad_table_chunks(table, n_tensors, "vs_grad_norm_tensors", true);
    if (chunks == (size_t)-1) return VS_ERR_INVALID;
    if (workspace_bytes < grad_ws_bytes(chunks))
        return vs_failf(VS_ERR_WORKSPACE, "vs_grad_norm_tensors: workspace %zu bytes < %zu needed", workspace_bytes, grad_ws_bytes(chunks));
    GradLauncher ln(kind, (double *)workspace, nullptr, stream);
    for (int i = 0; i < n_tensors; ++i) ln.add(table[i].g, table[i].n);
    return norm_finish(ln, kind, max_norm, grad_scale, out);
}

int vs_grad_norm(const vs_weights *w, const vs_model_grads *grads, int32_t kind, double max_norm, const float *grad_scale,
                 float *out, void *workspace, size_t workspace_bytes, void *stream) {
    if (!w || !grads) return vs_failf(VS_ERR_INVALID, "vs_grad_norm: weights/grads is NULL");
    if (int rc = check_norm_args("vs_grad_norm", kind, max_norm, out, workspace)) return rc;
    if (w->embedded())
        return vs_failf(VS_ERR_INVALID, "vs_grad_norm: the handle embeds a d_model=%d model in d_model=%d; use vs_grad_norm_tensors on the "
                                     "caller's tensors", w->dn(), w->desc.d_model);
    const int L = w->desc.num_layers, nt = handle_tensor_count(w);
    if (L > 0 && !grads->layers) return vs_failf(VS_ERR_INVALID, "vs_grad_norm: layers is NULL");
    auto grad_of = [&](int i) -> float * {
        if (i == 0) return grads->embed_w;
        if (i == 1) return grads->embed_b;
        if (i == 2 + 16 * L) return grads->final_w;
        if (i == 3 + 16 * L) return grads->final_b;
        return *layer_field(grads->layers[(i - 2) / 16], (i - 2) % 16);
    };
    size_t chunks = 0;
    for (int i = 0; i < nt; ++i)
        if (grad_of(i)) chunks += (handle_tensor(w, i).n + CHUNK - 1) / CHUNK;
    if (workspace_bytes < grad_ws_bytes(chunks))
        return vs_failf(VS_ERR_WORKSPACE, "vs_grad_norm: workspace %zu bytes < %zu needed", workspace_bytes, grad_ws_bytes(chunks));
    GradLauncher ln(kind, (double *)workspace, nullptr, stream);
    for (int i = 0; i < nt; ++i) ln.add(grad_of(i), handle_tensor(w, i).n);
    return norm_finish(ln, kind, max_norm, grad_scale, out);
}

int vs_grad_scale_tensors(const vs_grad_tensor *table, int32_t n_tensors, const float *coef, void *stream) {
    if (n_tensors < 0) return vs_failf(VS_ERR_INVALID, "vs_grad_scale_tensors: n_tensors=%d", n_tensors);
    if (!table) return vs_failf(VS_ERR_INVALID, "vs_grad_scale_tensors: table is NULL");
    if (!coef) return vs_failf(VS_ERR_INVALID, "vs_grad_scale_tensors: coef is NULL");
    if (grad_table_chunks(table, n_tensors, "vs_grad_scale_tensors", true) == (size_t)-1) return VS_ERR_INVALID;
    GradLauncher ln(VS_GRAD_NORM_L2, nullptr, coef, stream);
    for (int i = 0; i < n_tensors; ++i) ln.add(table[i].g, table[i].n);
    ln.flush();
    if (ln.err != hipSuccess) return vs_failf(VS_ERR_HIP, "grad scale launch failed: %s", hipGetErrorString(ln.err));
    return VS_OK;
}

}  // extern "C"
