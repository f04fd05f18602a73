// vs_pretrain_kernels.hip — the PretrainModel loss head on gfx950 (reference
// src/model/simnet_pretrain.py:49-69 repelling loss, :80-98 masked score-softmax pooling, centering penalty and the
// soft cross-entropy against the video representation), forward and backward.
//
// Per video b with frame features f_t (the video_transform output, F columns), scorer logits s_t and key mask:
//   w      = softmax_t(s_t / temp) over the unmasked frames                            :84-87
//   center = mean_t [unmasked] (w_t + 1e-9) log(w_t + 1e-9)   (entropy)  |  ||w||_2   (norm)      :88-92, 43-47
//   pooled = sum_t w_t f_t                                                             :93-95
//   loss   = mean_j -softmax(vid)_j log softmax(pooled)_j                              :96-97, 35-41
//   repel  = ( ||sum_t x^_t||^2 - sum_t ||x^_t||^2 ) / T^2,  x^_t = f_t [unmasked] / (||f_t|| + 1e-9)
//            = the mean of the off-diagonal of the reference's materialised [T,T] cosine matrix (:56-69) without the
//            matrix: O(T F) instead of O(T^2 F), forward and backward.
// The three returned losses are the means over the batch.  Everything is HBM-bound row work (one pass over the
// [B,T,F] features forward, two backward): a wave owns a frame, a lane 4 consecutive features per 256, and all sums
// are two-stage with fixed order (chunk partials -> per-video finals -> batch means), so results are reproducible.
#include "vs_train_device.h"
#include "vs_train_kernels.h"

namespace {

constexpr int CHUNK = 64;            // frames per block
constexpr float EPS = 1e-9f;         // the reference's stabilisers (:55, :90)
enum { ST_M = 0, ST_Z, ST_D, ST_CEN, ST_R, ST_W2, ST_N = 8 };     // per-video scalars

struct Layout {                      // scratch carving (floats)
    size_t stats, pooled, sumx, dce, part, rpart, a, total;
    int nc;
};
__host__ __device__ inline Layout layout(int B, int T, int F) {
    Layout L;
    L.nc = (T + CHUNK - 1) / CHUNK;
    size_t off = 0;
    L.stats = off; off += (size_t)B * ST_N;
    L.pooled = off; off += (size_t)B * F;
    L.sumx = off; off += (size_t)B * F;
    L.dce = off; off += (size_t)B * F;
    L.part = off; off += (size_t)B * L.nc * (2 * F + 4);
    L.rpart = off; off += (size_t)B * L.nc;
    L.a = off; off += (size_t)B * T;
    L.total = off;
    return L;
}

// block-wide max and sum-exp of the video's scaled, masked scores (every block recomputes them: T <= a few thousand)
__device__ __forceinline__ void softmax_stats(const float *__restrict__ s, const uint8_t *__restrict__ mk, int T,
                                              float inv_temp, float &m, float &Z, float *red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float mx = -__builtin_inff();
    for (int t = tid; t < T; t += 256)
        if (!mk || !mk[t]) mx = fmaxf(mx, s[t] * inv_temp);
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float z = 0.f;
    for (int t = tid; t < T; t += 256)
        if (!mk || !mk[t]) z += expf(s[t] * inv_temp - m);
    z = wave_sum(z);
    if (lane == 0) red[wave] = z;
    __syncthreads();
    Z = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
}

// ---- forward, stage 1: per (video, 64-frame chunk) partial sums ----
template <int NV>       // F = 256 * NV
__global__ __launch_bounds__(256) void head_partial(const float *__restrict__ feats, const float *__restrict__ scores,
                                                    const uint8_t *__restrict__ mask, int T, float inv_temp, int entropy,
                                                    float *__restrict__ scratch, int B) {
    constexpr int F = 256 * NV;
    __shared__ float red[4][2 * F + 4];
    __shared__ float sred[4];
    const Layout L = layout(B, T, F);
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *s = scores + (size_t)b * T;
    const uint8_t *mk = mask ? mask + (size_t)b * T : nullptr;
    float m, Z;
    softmax_stats(s, mk, T, inv_temp, m, Z, sred);
    f32x4 pool[NV], sx[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) { pool[u] = f32x4{0.f, 0.f, 0.f, 0.f}; sx[u] = pool[u]; }
    float dsum = 0.f, cen = 0.f;
    for (int t = ch * CHUNK + wave; t < min(T, (ch + 1) * CHUNK); t += 4) {
        const bool valid = !mk || !mk[t];
        const float w = valid ? expf(s[t] * inv_temp - m) / Z : 0.f;
        f32x4 f[NV];
        float nn = 0.f;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            f[u] = *(const f32x4 *)(feats + ((size_t)b * T + t) * F + 4 * lane + 256 * u);
            nn += f[u][0] * f[u][0] + f[u][1] * f[u][1] + f[u][2] * f[u][2] + f[u][3] * f[u][3];
            pool[u] += f[u] * w;
        }
        if (valid) {
            const float n = sqrtf(wave_sum(nn)), inv = 1.0f / (n + EPS);
#pragma unroll
            for (int u = 0; u < NV; ++u) sx[u] += f[u] * inv;
            dsum += (n * inv) * (n * inv);
            cen += entropy ? (w + EPS) * logf(w + EPS) : w * w;      // masked frames: masked_fill(mask, 0.) (:46) / w = 0
        }
    }
#pragma unroll
    for (int u = 0; u < NV; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            red[wave][4 * lane + 256 * u + e] = pool[u][e];
            red[wave][F + 4 * lane + 256 * u + e] = sx[u][e];
        }
    if (lane == 0) { red[wave][2 * F] = dsum; red[wave][2 * F + 1] = cen; }
    __syncthreads();
    float *out = scratch + L.part + ((size_t)b * L.nc + ch) * (2 * F + 4);
    for (int i = tid; i < 2 * F + 2; i += 256) out[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// ---- forward, stage 2: per-video finals ----
template <int NV>
__global__ __launch_bounds__(256) void head_final(const float *__restrict__ scores, const uint8_t *__restrict__ mask,
                                                  const float *__restrict__ vid, int T, float inv_temp, int entropy,
                                                  float *__restrict__ scratch, int B) {
    constexpr int F = 256 * NV;
    __shared__ float sred[4];
    __shared__ float vec[3][F];            // pooled, sumx, vid
    const Layout L = layout(B, T, F);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float m, Z;
    softmax_stats(scores + (size_t)b * T, mask ? mask + (size_t)b * T : nullptr, T, inv_temp, m, Z, sred);
    const float *part = scratch + L.part + (size_t)b * L.nc * (2 * F + 4);
    for (int i = tid; i < 2 * F; i += 256) {
        float acc = 0.f;
        for (int c = 0; c < L.nc; ++c) acc += part[(size_t)c * (2 * F + 4) + i];
        vec[i / F][i % F] = acc;
        if (i < F) scratch[L.pooled + (size_t)b * F + i] = acc;
        else scratch[L.sumx + (size_t)b * F + (i - F)] = acc;
    }
    for (int i = tid; i < F; i += 256) vec[2][i] = vid[(size_t)b * F + i];
    __syncthreads();
    // block reductions (fixed order: per-thread stride, wave shuffle tree, 4 waves in order)
    auto block_sum = [&](float v) {
        v = wave_sum(v);
        if (lane == 0) sred[wave] = v;
        __syncthreads();
        const float r = ((sred[0] + sred[1]) + sred[2]) + sred[3];
        __syncthreads();
        return r;
    };
    auto block_max = [&](float v) {
        for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
        if (lane == 0) sred[wave] = v;
        __syncthreads();
        const float r = fmaxf(fmaxf(sred[0], sred[1]), fmaxf(sred[2], sred[3]));
        __syncthreads();
        return r;
    };
    float ss = 0.f, mp = -__builtin_inff(), mv = -__builtin_inff();
    for (int i = tid; i < F; i += 256) { ss += vec[1][i] * vec[1][i]; mp = fmaxf(mp, vec[0][i]); mv = fmaxf(mv, vec[2][i]); }
    const float S2 = block_sum(ss);
    mp = block_max(mp); mv = block_max(mv);
    float zp = 0.f, zv = 0.f;
    for (int i = tid; i < F; i += 256) { zp += expf(vec[0][i] - mp); zv += expf(vec[2][i] - mv); }
    zp = block_sum(zp); zv = block_sum(zv);
    const float lzp = logf(zp);
    float ce = 0.f;
    for (int i = tid; i < F; i += 256) {
        const float p2 = expf(vec[2][i] - mv) / zv, logp1 = vec[0][i] - mp - lzp;
        ce -= p2 * logp1;
        scratch[L.dce + (size_t)b * F + i] = expf(logp1) - p2;        // d CE_b / d pooled_i (before the 1/(B F) of the mean)
    }
    ce = block_sum(ce);
    // every frame masked: the reference's softmax over -inf is NaN, and so are its pooled row, its distillation loss, its
    // norm penalty and every gradient through them (entropy: masked_fill(mask, 0.) leaves 0).  The sums above saw w = 0.
    const bool dead = !(Z > 0.f);
    if (dead)
        for (int i = tid; i < F; i += 256) scratch[L.dce + (size_t)b * F + i] = __builtin_nanf("");
    if (tid == 0) {
        float D = 0.f, cen = 0.f;
        for (int c = 0; c < L.nc; ++c) { D += part[(size_t)c * (2 * F + 4) + 2 * F]; cen += part[(size_t)c * (2 * F + 4) + 2 * F + 1]; }
        float *st = scratch + L.stats + (size_t)b * ST_N;
        st[ST_M] = m; st[ST_Z] = Z; st[ST_D] = D;
        st[ST_W2] = cen;                                       // norm penalty: sum of w^2
        st[ST_CEN] = entropy ? cen / (float)T : sqrtf(cen);    // per-video centering value
        st[ST_R] = (S2 - D) / ((float)T * (float)T);           // per-video repel value
        st[ST_N - 1] = ce / (float)F;                          // per-video distillation loss
        if (dead) { st[ST_N - 1] = __builtin_nanf(""); if (!entropy) st[ST_CEN] = __builtin_nanf(""); }
    }
}

// losses[0..2] = batch means of (distillation, centering, repel)
__global__ void head_losses(const float *__restrict__ scratch, int B, int T, int F, float *__restrict__ losses) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const Layout L = layout(B, T, F);
    float a = 0.f, c = 0.f, r = 0.f;
    for (int b = 0; b < B; ++b) {
        const float *st = scratch + L.stats + (size_t)b * ST_N;
        a += st[ST_N - 1]; c += st[ST_CEN]; r += st[ST_R];
    }
    losses[0] = a / (float)B; losses[1] = c / (float)B; losses[2] = r / (float)B;
}

// ---- backward, stage 1: a_t = d_pooled . f_t and the chunk partial of R = sum_t w_t * d w_t ----
template <int NV>
__global__ __launch_bounds__(256) void head_bwd_dots(const float *__restrict__ feats, const float *__restrict__ scores,
                                                     const uint8_t *__restrict__ mask, int T, float inv_temp, int entropy,
                                                     float *__restrict__ scratch, const float *__restrict__ g, int B) {
    constexpr int F = 256 * NV;
    __shared__ float sred[4];
    const Layout L = layout(B, T, F);
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *st = scratch + L.stats + (size_t)b * ST_N;
    const float m = st[ST_M], Z = st[ST_Z];
    const uint8_t *mk = mask ? mask + (size_t)b * T : nullptr;
    const float gl = g[0] / ((float)B * (float)F), gc = g[1] / (float)B;
    f32x4 dp[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) dp[u] = *(const f32x4 *)(scratch + L.dce + (size_t)b * F + 4 * lane + 256 * u) * gl;
    float racc = 0.f;
    for (int t = ch * CHUNK + wave; t < min(T, (ch + 1) * CHUNK); t += 4) {
        float dot = 0.f;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const f32x4 f = *(const f32x4 *)(feats + ((size_t)b * T + t) * F + 4 * lane + 256 * u);
            dot += f[0] * dp[u][0] + f[1] * dp[u][1] + f[2] * dp[u][2] + f[3] * dp[u][3];
        }
        dot = wave_sum(dot);
        const bool valid = !mk || !mk[t];
        const float w = valid ? expf(scores[(size_t)b * T + t] * inv_temp - m) / Z : 0.f;
        float dw = dot;
        // (one fused multiply-add, spelled out: head_bwd_dots_pk must round the same way)
        if (entropy) { if (valid) dw = __builtin_fmaf(gc / (float)T, logf(w + EPS) + 1.0f, dw); }
        else dw += gc * w / sqrtf(st[ST_W2]);
        if (lane == 0) { scratch[L.a + (size_t)b * T + t] = dw; racc += w * dw; }
    }
    if (lane == 0) sred[wave] = racc;
    __syncthreads();
    if (tid == 0) scratch[L.rpart + (size_t)b * L.nc + ch] = ((sred[0] + sred[1]) + sred[2]) + sred[3];
}

// ---- backward, stage 2: d_scores and d_feats ----
template <int NV>
__global__ __launch_bounds__(256) void head_bwd_final(const float *__restrict__ feats, const float *__restrict__ scores,
                                                      const uint8_t *__restrict__ mask, int T, float inv_temp,
                                                      const float *__restrict__ scratch, const float *__restrict__ g,
                                                      float *__restrict__ d_feats, float *__restrict__ d_scores, int B) {
    constexpr int F = 256 * NV;
    const Layout L = layout(B, T, F);
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *st = scratch + L.stats + (size_t)b * ST_N;
    const float m = st[ST_M], Z = st[ST_Z];
    const uint8_t *mk = mask ? mask + (size_t)b * T : nullptr;
    float R = 0.f;
    for (int c = 0; c < L.nc; ++c) R += scratch[L.rpart + (size_t)b * L.nc + c];
    const float gl = g[0] / ((float)B * (float)F), coef = 2.0f * g[2] / ((float)B * (float)T * (float)T);
    f32x4 dp[NV], S[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        dp[u] = *(const f32x4 *)(scratch + L.dce + (size_t)b * F + 4 * lane + 256 * u) * gl;
        S[u] = *(const f32x4 *)(scratch + L.sumx + (size_t)b * F + 4 * lane + 256 * u);
    }
    for (int t = ch * CHUNK + wave; t < min(T, (ch + 1) * CHUNK); t += 4) {
        const bool valid = !mk || !mk[t];
        const float w = valid ? expf(scores[(size_t)b * T + t] * inv_temp - m) / Z : 0.f;
        const float dw = scratch[L.a + (size_t)b * T + t];
        if (lane == 0) d_scores[(size_t)b * T + t] = w * (dw - R) * inv_temp;
        f32x4 f[NV], out[NV];
        float nn = 0.f;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            f[u] = *(const f32x4 *)(feats + ((size_t)b * T + t) * F + 4 * lane + 256 * u);
            nn += f[u][0] * f[u][0] + f[u][1] * f[u][1] + f[u][2] * f[u][2] + f[u][3] * f[u][3];
            out[u] = dp[u] * w;
        }
        nn = wave_sum(nn);
        if (valid && nn > 0.f) {
            // x^ = f / (n + eps):  d f = v / (n + eps) - f (f . v) / (n (n + eps)^2),  v = coef * (S - x^)
            const float n = sqrtf(nn), inv = 1.0f / (n + EPS);
            float fv = 0.f;
            f32x4 v[NV];
#pragma unroll
            for (int u = 0; u < NV; ++u) {
                v[u] = (S[u] - f[u] * inv) * coef;
                fv += f[u][0] * v[u][0] + f[u][1] * v[u][1] + f[u][2] * v[u][2] + f[u][3] * v[u][3];
            }
            fv = wave_sum(fv);
            const float k2 = fv * inv * inv / n;
#pragma unroll
            for (int u = 0; u < NV; ++u) out[u] += v[u] * inv - f[u] * k2;
        }
#pragma unroll
        for (int u = 0; u < NV; ++u) *(f32x4 *)(d_feats + ((size_t)b * T + t) * F + 4 * lane + 256 * u) = out[u];
    }
}

}  // namespace

size_t vsp_head_scratch_floats(int B, int T, int F) { return layout(B, T, F).total; }

int vsp_head_forward(const float *feats, const float *scores, const uint8_t *mask, const float *vid, int B, int T, int F,
                     float inv_temp, int entropy_penalty, float *scratch, float *losses, hipStream_t st) {
    if (F != 256 && F != 512 && F != 768 && F != 1024) return -1;
    const Layout L = layout(B, T, F);
    const dim3 grid(L.nc, B);
#define VSP_CASE(NV_)                                                                                                    \
    case NV_:                                                                                                            \
        hipLaunchKernelGGL(head_partial<NV_>, grid, dim3(256), 0, st, feats, scores, mask, T, inv_temp, entropy_penalty, scratch, B); \
        hipLaunchKernelGGL(head_final<NV_>, dim3(B), dim3(256), 0, st, scores, mask, vid, T, inv_temp, entropy_penalty, scratch, B);   \
        break;
    switch (F / 256) { VSP_CASE(1) VSP_CASE(2) VSP_CASE(3) VSP_CASE(4) default: return -1; }
#undef VSP_CASE
    VSK_CHECK_LAUNCH();
    hipLaunchKernelGGL(head_losses, dim3(1), dim3(64), 0, st, scratch, B, T, F, losses);
    VSK_CHECK_LAUNCH();
    return 0;
}

int vsp_head_backward(const float *feats, const float *scores, const uint8_t *mask, const float *vid, int B, int T, int F,
                      float inv_temp, int entropy_penalty, const float *scratch, const float *g_losses, float *d_feats,
                      float *d_scores, hipStream_t st) {
    (void)vid;
    if (F != 256 && F != 512 && F != 768 && F != 1024) return -1;
    const Layout L = layout(B, T, F);
    const dim3 grid(L.nc, B);
    float *sc = const_cast<float *>(scratch);      // the a / rpart regions are backward-only scratch
#define VSP_CASE(NV_)                                                                                                    \
    case NV_:                                                                                                            \
        hipLaunchKernelGGL(head_bwd_dots<NV_>, grid, dim3(256), 0, st, feats, scores, mask, T, inv_temp, entropy_penalty, sc, g_losses, B); \
        hipLaunchKernelGGL(head_bwd_final<NV_>, grid, dim3(256), 0, st, feats, scores, mask, T, inv_temp, scratch, g_losses, d_feats, d_scores, B); \
        break;
    switch (F / 256) { VSP_CASE(1) VSP_CASE(2) VSP_CASE(3) VSP_CASE(4) default: return -1; }
#undef VSP_CASE
    VSK_CHECK_LAUNCH();
    return 0;
}

// ---- packed ragged batches (vs_pretrain_head_forward_packed): feats [Mtot,F] and scores [Mtot] hold the frames of B videos
// concatenated, there is no mask, and the denominators of the centering mean and of the repelling loss are the reference's
// padded width Tref (>= the longest video), so values and gradients are those of the padded batch of the same videos.
// The kernels above stay as they are; these are their counterparts, with the same per-frame arithmetic, lane ownership and
// summation order.  A block owns one 64-frame chunk of ONE video (chunks are counted per video, so none straddles two), and
// finds it from the device lengths alone: every wave scans them (B values, 64 per step) - no plan is stored, nothing is read
// from the host after the launch.  Lengths are cut at `tmax`, rows beyond Mtot and chunks beyond `NC` (both as the host
// counted them) are cut, so device lengths that disagree with the host's cannot move a write outside the buffers the host sized.
namespace {

struct PkArgs { const int *len; int B, Mtot, tmax, NC; float tref; };
struct PkLayout { size_t stats, pooled, sumx, dce, part, rpart, a, total; };
__host__ __device__ inline PkLayout layout_pk(int B, int Mtot, int NC, int F) {
    PkLayout L;
    size_t off = 0;
    L.stats = off; off += (size_t)B * ST_N;
    L.pooled = off; off += (size_t)B * F;
    L.sumx = off; off += (size_t)B * F;
    L.dce = off; off += (size_t)B * F;
    L.part = off; off += (size_t)NC * (2 * F + 4);
    L.rpart = off; off += (size_t)NC;
    L.a = off; off += (size_t)Mtot;
    L.total = off;
    return L;
}

struct PkLoc { int b, row0, T, cbase, ch; };      // video, its first packed row, its frames, its first chunk, the chunk within it

// the video that owns chunk g (want_b < 0), or video want_b; the same answer in every lane of every wave.  b = -1: none.
__device__ __forceinline__ PkLoc pk_locate(const PkArgs &A, int g, int want_b) {
    const int lane = threadIdx.x & 63;
    long long rows = 0;
    int chunks = 0;
    PkLoc L{-1, 0, 0, 0, 0};
    for (int base = 0; base < A.B; base += 64) {
        const int i = base + lane;
        const int t = i < A.B ? min(max(A.len[i], 0), A.tmax) : 0;
        long long incl = t;
        for (int off = 1; off < 64; off <<= 1) { const long long u = __shfl_up(incl, off); if (lane >= off) incl += u; }
        incl += rows;
        const int r1 = (int)min(incl, (long long)A.Mtot), r0 = (int)min(incl - t, (long long)A.Mtot), tt = r1 - r0;
        const int nch = (tt + CHUNK - 1) / CHUNK;
        int ic = nch;
        for (int off = 1; off < 64; off <<= 1) { const int u = __shfl_up(ic, off); if (lane >= off) ic += u; }
        ic += chunks;
        const int ec = ic - nch;
        const bool mine = want_b >= 0 ? i == want_b : (g >= ec && g < ic);
        const unsigned long long found = __ballot(mine);
        if (found) {
            const int src = __ffsll((long long)found) - 1;
            L.b = base + src; L.row0 = __shfl(r0, src); L.T = __shfl(tt, src); L.cbase = __shfl(ec, src); L.ch = g - L.cbase;
            return L;
        }
        rows = __shfl(incl, 63); chunks = __shfl(ic, 63);
    }
    return L;
}

// ---- forward, stage 1: one block per (video, 64-frame chunk) ----
template <int NV>
__global__ __launch_bounds__(256) void head_partial_pk(const float *__restrict__ feats, const float *__restrict__ scores,
                                                       const PkArgs A, float inv_temp, int entropy, float *__restrict__ scratch) {
    constexpr int F = 256 * NV;
    __shared__ float red[4][2 * F + 4];
    __shared__ float sred[4];
    const PkLayout L = layout_pk(A.B, A.Mtot, A.NC, F);
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PkLoc V = pk_locate(A, g, -1);
    if (V.b < 0) return;
    const int T = V.T, ch = V.ch;
    const float *s = scores + V.row0;
    const float *fv = feats + (size_t)V.row0 * F;
    float m, Z;
    softmax_stats(s, nullptr, T, inv_temp, m, Z, sred);
    f32x4 pool[NV], sx[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) { pool[u] = f32x4{0.f, 0.f, 0.f, 0.f}; sx[u] = pool[u]; }
    float dsum = 0.f, cen = 0.f;
    for (int t = ch * CHUNK + wave; t < min(T, (ch + 1) * CHUNK); t += 4) {
        const float w = expf(s[t] * inv_temp - m) / Z;
        f32x4 f[NV];
        float nn = 0.f;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            f[u] = *(const f32x4 *)(fv + (size_t)t * F + 4 * lane + 256 * u);
            nn += f[u][0] * f[u][0] + f[u][1] * f[u][1] + f[u][2] * f[u][2] + f[u][3] * f[u][3];
            pool[u] += f[u] * w;
        }
        const float n = sqrtf(wave_sum(nn)), inv = 1.0f / (n + EPS);
#pragma unroll
        for (int u = 0; u < NV; ++u) sx[u] += f[u] * inv;
        dsum += (n * inv) * (n * inv);
        cen += entropy ? (w + EPS) * logf(w + EPS) : w * w;
    }
#pragma unroll
    for (int u = 0; u < NV; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            red[wave][4 * lane + 256 * u + e] = pool[u][e];
            red[wave][F + 4 * lane + 256 * u + e] = sx[u][e];
        }
    if (lane == 0) { red[wave][2 * F] = dsum; red[wave][2 * F + 1] = cen; }
    __syncthreads();
    float *out = scratch + L.part + (size_t)g * (2 * F + 4);
    for (int i = tid; i < 2 * F + 2; i += 256) out[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// ---- forward, stage 2: one block per video ----
template <int NV>
__global__ __launch_bounds__(256) void head_final_pk(const float *__restrict__ scores, const float *__restrict__ vid,
                                                     const PkArgs A, float inv_temp, int entropy, float *__restrict__ scratch) {
    constexpr int F = 256 * NV;
    __shared__ float sred[4];
    __shared__ float vec[3][F];            // pooled, sumx, vid
    const PkLayout L = layout_pk(A.B, A.Mtot, A.NC, F);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PkLoc V = pk_locate(A, 0, b);
    const int T = V.T;
    const int nc = max(0, min((T + CHUNK - 1) / CHUNK, A.NC - V.cbase));      // the chunks stage 1 ran
    float m, Z;
    softmax_stats(scores + V.row0, nullptr, T, inv_temp, m, Z, sred);
    const float *part = scratch + L.part + (size_t)V.cbase * (2 * F + 4);
    for (int i = tid; i < 2 * F; i += 256) {
        float acc = 0.f;
        for (int c = 0; c < nc; ++c) acc += part[(size_t)c * (2 * F + 4) + i];
        vec[i / F][i % F] = acc;
        if (i < F) scratch[L.pooled + (size_t)b * F + i] = acc;
        else scratch[L.sumx + (size_t)b * F + (i - F)] = acc;
    }
    for (int i = tid; i < F; i += 256) vec[2][i] = vid[(size_t)b * F + i];
    __syncthreads();
    auto block_sum = [&](float v) {
        v = wave_sum(v);
        if (lane == 0) sred[wave] = v;
        __syncthreads();
        const float r = ((sred[0] + sred[1]) + sred[2]) + sred[3];
        __syncthreads();
        return r;
    };
    auto block_max = [&](float v) {
        for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
        if (lane == 0) sred[wave] = v;
        __syncthreads();
        const float r = fmaxf(fmaxf(sred[0], sred[1]), fmaxf(sred[2], sred[3]));
        __syncthreads();
        return r;
    };
    float ss = 0.f, mp = -__builtin_inff(), mv = -__builtin_inff();
    for (int i = tid; i < F; i += 256) { ss += vec[1][i] * vec[1][i]; mp = fmaxf(mp, vec[0][i]); mv = fmaxf(mv, vec[2][i]); }
    const float S2 = block_sum(ss);
    mp = block_max(mp); mv = block_max(mv);
    float zp = 0.f, zv = 0.f;
    for (int i = tid; i < F; i += 256) { zp += expf(vec[0][i] - mp); zv += expf(vec[2][i] - mv); }
    zp = block_sum(zp); zv = block_sum(zv);
    const float lzp = logf(zp);
    float ce = 0.f;
    for (int i = tid; i < F; i += 256) {
        const float p2 = expf(vec[2][i] - mv) / zv, logp1 = vec[0][i] - mp - lzp;
        ce -= p2 * logp1;
        scratch[L.dce + (size_t)b * F + i] = expf(logp1) - p2;
    }
    ce = block_sum(ce);
    if (tid == 0) {
        float D = 0.f, cen = 0.f;
        for (int c = 0; c < nc; ++c) { D += part[(size_t)c * (2 * F + 4) + 2 * F]; cen += part[(size_t)c * (2 * F + 4) + 2 * F + 1]; }
        float *st = scratch + L.stats + (size_t)b * ST_N;
        st[ST_M] = m; st[ST_Z] = Z; st[ST_D] = D;
        st[ST_W2] = cen;
        st[ST_CEN] = entropy ? cen / A.tref : sqrtf(cen);      // the reference's mean(dim=1) divides by the padded width
        st[ST_R] = (S2 - D) / (A.tref * A.tref);               // ... and so does its [T,T] mean
        st[ST_N - 1] = ce / (float)F;
    }
}

__global__ void head_losses_pk(const float *__restrict__ stats, int B, float *__restrict__ losses) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float a = 0.f, c = 0.f, r = 0.f;
    for (int b = 0; b < B; ++b) {
        const float *st = stats + (size_t)b * ST_N;
        a += st[ST_N - 1]; c += st[ST_CEN]; r += st[ST_R];
    }
    losses[0] = a / (float)B; losses[1] = c / (float)B; losses[2] = r / (float)B;
}

// ---- backward, stage 1 ----
template <int NV>
__global__ __launch_bounds__(256) void head_bwd_dots_pk(const float *__restrict__ feats, const float *__restrict__ scores,
                                                        const PkArgs A, float inv_temp, int entropy, float *__restrict__ scratch,
                                                        const float *__restrict__ g) {
    constexpr int F = 256 * NV;
    __shared__ float sred[4];
    const PkLayout L = layout_pk(A.B, A.Mtot, A.NC, F);
    const int gi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PkLoc V = pk_locate(A, gi, -1);
    if (V.b < 0) return;
    const int b = V.b, T = V.T, ch = V.ch;
    const float *st = scratch + L.stats + (size_t)b * ST_N;
    const float m = st[ST_M], Z = st[ST_Z];
    const float gl = g[0] / ((float)A.B * (float)F), gc = g[1] / (float)A.B;
    f32x4 dp[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) dp[u] = *(const f32x4 *)(scratch + L.dce + (size_t)b * F + 4 * lane + 256 * u) * gl;
    float racc = 0.f;
    for (int t = ch * CHUNK + wave; t < min(T, (ch + 1) * CHUNK); t += 4) {
        const size_t row = (size_t)V.row0 + t;
        float dot = 0.f;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const f32x4 f = *(const f32x4 *)(feats + row * F + 4 * lane + 256 * u);
            dot += f[0] * dp[u][0] + f[1] * dp[u][1] + f[2] * dp[u][2] + f[3] * dp[u][3];
        }
        dot = wave_sum(dot);
        const float w = expf(scores[row] * inv_temp - m) / Z;
        float dw = dot;
        // fused like head_bwd_dots: left to the compiler this was a multiply and an add after the join with the norm branch,
        // one rounding more than the padded kernel, and d_logits differed in the last bit under the entropy penalty
        if (entropy) dw = __builtin_fmaf(gc / A.tref, logf(w + EPS) + 1.0f, dw);
        else dw += gc * w / sqrtf(st[ST_W2]);
        if (lane == 0) { scratch[L.a + row] = dw; racc += w * dw; }
    }
    if (lane == 0) sred[wave] = racc;
    __syncthreads();
    if (tid == 0) scratch[L.rpart + gi] = ((sred[0] + sred[1]) + sred[2]) + sred[3];
}

// ---- backward, stage 2 ----
template <int NV>
__global__ __launch_bounds__(256) void head_bwd_final_pk(const float *__restrict__ feats, const float *__restrict__ scores,
                                                         const PkArgs A, float inv_temp, const float *__restrict__ scratch,
                                                         const float *__restrict__ g, float *__restrict__ d_feats,
                                                         float *__restrict__ d_scores) {
    constexpr int F = 256 * NV;
    const PkLayout L = layout_pk(A.B, A.Mtot, A.NC, F);
    const int gi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PkLoc V = pk_locate(A, gi, -1);
    if (V.b < 0) return;
    const int b = V.b, T = V.T, ch = V.ch;
    const float *st = scratch + L.stats + (size_t)b * ST_N;
    const float m = st[ST_M], Z = st[ST_Z];
    const int nc = min((T + CHUNK - 1) / CHUNK, A.NC - V.cbase);
    float R = 0.f;
    for (int c = 0; c < nc; ++c) R += scratch[L.rpart + V.cbase + c];
    const float gl = g[0] / ((float)A.B * (float)F), coef = 2.0f * g[2] / ((float)A.B * A.tref * A.tref);
    f32x4 dp[NV], S[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        dp[u] = *(const f32x4 *)(scratch + L.dce + (size_t)b * F + 4 * lane + 256 * u) * gl;
        S[u] = *(const f32x4 *)(scratch + L.sumx + (size_t)b * F + 4 * lane + 256 * u);
    }
    for (int t = ch * CHUNK + wave; t < min(T, (ch + 1) * CHUNK); t += 4) {
        const size_t row = (size_t)V.row0 + t;
        const float w = expf(scores[row] * inv_temp - m) / Z;
        const float dw = scratch[L.a + row];
        if (lane == 0) d_scores[row] = w * (dw - R) * inv_temp;
        f32x4 f[NV], out[NV];
        float nn = 0.f;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            f[u] = *(const f32x4 *)(feats + row * F + 4 * lane + 256 * u);
            nn += f[u][0] * f[u][0] + f[u][1] * f[u][1] + f[u][2] * f[u][2] + f[u][3] * f[u][3];
            out[u] = dp[u] * w;
        }
        nn = wave_sum(nn);
        if (nn > 0.f) {
            const float n = sqrtf(nn), inv = 1.0f / (n + EPS);
            float fv = 0.f;
            f32x4 v[NV];
#pragma unroll
            for (int u = 0; u < NV; ++u) {
                v[u] = (S[u] - f[u] * inv) * coef;
                fv += f[u][0] * v[u][0] + f[u][1] * v[u][1] + f[u][2] * v[u][2] + f[u][3] * v[u][3];
            }
            fv = wave_sum(fv);
            const float k2 = fv * inv * inv / n;
#pragma unroll
            for (int u = 0; u < NV; ++u) out[u] += v[u] * inv - f[u] * k2;
        }
#pragma unroll
        for (int u = 0; u < NV; ++u) *(f32x4 *)(d_feats + row * F + 4 * lane + 256 * u) = out[u];
    }
}

}  // namespace

size_t vsp_head_scratch_floats_packed(int B, int Mtot, int NC, int F) { return layout_pk(B, Mtot, NC, F).total; }

int vsp_head_forward_packed(const float *feats, const float *scores, const int *lengths_dev, const float *vid, int B, int Mtot,
                            int tmax, int NC, int ref_len, int F, float inv_temp, int entropy_penalty, float *scratch,
                            float *losses, hipStream_t st) {
    if (F != 256 && F != 512 && F != 768 && F != 1024) return -1;
    const PkArgs A{lengths_dev, B, Mtot, tmax, NC, (float)ref_len};
#define VSP_CASE(NV_)                                                                                                    \
    case NV_:                                                                                                            \
        hipLaunchKernelGGL(head_partial_pk<NV_>, dim3(NC), dim3(256), 0, st, feats, scores, A, inv_temp, entropy_penalty, scratch); \
        hipLaunchKernelGGL(head_final_pk<NV_>, dim3(B), dim3(256), 0, st, scores, vid, A, inv_temp, entropy_penalty, scratch);      \
        break;
    switch (F / 256) { VSP_CASE(1) VSP_CASE(2) VSP_CASE(3) VSP_CASE(4) default: return -1; }
#undef VSP_CASE
    VSK_CHECK_LAUNCH();
    hipLaunchKernelGGL(head_losses_pk, dim3(1), dim3(64), 0, st, scratch + layout_pk(B, Mtot, NC, F).stats, B, losses);
    VSK_CHECK_LAUNCH();
    return 0;
}

int vsp_head_backward_packed(const float *feats, const float *scores, const int *lengths_dev, int B, int Mtot, int tmax, int NC,
                             int ref_len, int F, float inv_temp, int entropy_penalty, float *scratch, const float *g_losses,
                             float *d_feats, float *d_scores, hipStream_t st) {
    if (F != 256 && F != 512 && F != 768 && F != 1024) return -1;
    const PkArgs A{lengths_dev, B, Mtot, tmax, NC, (float)ref_len};
#define VSP_CASE(NV_)                                                                                                    \
    case NV_:                                                                                                            \
        hipLaunchKernelGGL(head_bwd_dots_pk<NV_>, dim3(NC), dim3(256), 0, st, feats, scores, A, inv_temp, entropy_penalty, scratch, g_losses); \
        hipLaunchKernelGGL(head_bwd_final_pk<NV_>, dim3(NC), dim3(256), 0, st, feats, scores, A, inv_temp, scratch, g_losses, d_feats, d_scores); \
        break;
    switch (F / 256) { VSP_CASE(1) VSP_CASE(2) VSP_CASE(3) VSP_CASE(4) default: return -1; }
#undef VSP_CASE
    VSK_CHECK_LAUNCH();
    return 0;
}
