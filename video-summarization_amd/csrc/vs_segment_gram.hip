// Kernel temporal segmentation (KTS) on gfx950: the ragged-batch symmetric Gram with its kernel epilogue, and the score of
// given change points.
//
// Gram: ONE launch for the whole batch.  A block owns one 64 x 64 tile (tile row >= tile column) of one video's
// K = X X^T; the block index is a position in the concatenated lower-triangle tile lists of the videos (found by a binary
// search over KtsGramVideo::tile0).  The operands are read straight from the caller's packed X (row stride D): rows past
// n and columns past D are zero in the loads, so there is no padded copy.  A 64 x 32 chunk of each operand goes through
// LDS (row stride 33: the 32 lanes of a half-wave read 32 rows of one column from 32 banks); each of the four waves owns
// one 32 x 32 quadrant on v_mfma_f32_32x32x2_f32, k ascending - the exact fp32 fma chain of the GEMMs.  The epilogue
// (none / cosine / rbf, in double) is applied to the accumulator; every element with row >= column is stored, and stored
// again at its mirror through an LDS transpose (both stores 128-byte rows), so K is symmetric bit for bit.  In a diagonal
// tile the upper-right quadrant is the mirror of the lower-left one and is not computed.
// A value depends only on its two rows of X and on D, never on the batch around it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vs_device.h"
#include "vs_segment_kernels.h"

namespace {

constexpr int GT = 64;                  // tile edge
constexpr int GK = 32;                  // k per LDS chunk
constexpr int GLD = GK + 1;             // LDS row stride of an operand chunk
constexpr int GNT = 256;                // threads per block: four waves, one 32 x 32 quadrant each
constexpr int TLD = GT + 1;             // LDS row stride of the transposed tile
constexpr int KTS_BLOB_WORDS = 896;     // 3584 bytes of kernel arguments per put launch

struct KtsBlob { int32_t w[KTS_BLOB_WORDS]; };

// host bytes -> device memory as kernel ARGUMENTS: stream-ordered, and the host buffer is free once the launch returns
__global__ __launch_bounds__(GNT) void kts_put(KtsBlob blob, int32_t *__restrict__ dst, int words) {
    for (int i = threadIdx.x; i < words; i += GNT) dst[i] = blob.w[i];
}

// one wave per row: s = sum_k x_k^2 in double, lane l takes k = l, l + 64, ... ascending, then the xor tree.
// mode 0: out = s; mode 1: out = s > 0 ? 1 / sqrt(s) : 0
__global__ __launch_bounds__(GNT) void kts_row_norms(const float *__restrict__ x, int d, int rows, int mode,
                                                     double *__restrict__ out) {
    const int row = blockIdx.x * (GNT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float *xr = x + (size_t)row * d;
    double s = 0.0;
    for (int k = lane; k < d; k += 64) {
        const double v = (double)xr[k];
        s += v * v;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) out[row] = mode == 0 ? s : (s > 0.0 ? 1.0 / sqrt(s) : 0.0);
}

// idx -> (ti, tj), tj <= ti, idx = ti (ti + 1) / 2 + tj
__device__ inline void tri_decode(int idx, int &ti, int &tj) {
    int t = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
    while ((t + 1) * (t + 2) / 2 <= idx) ++t;
    while (t * (t + 1) / 2 > idx) --t;
    ti = t;
    tj = idx - t * (t + 1) / 2;
}

// chunk k0 of rows [r0, r0 + 64) of video rows xv[0 .. n): VEC = 1: thread t takes k = t & 31 of rows (t >> 5) + 8 q;
// VEC = 4 (d % 4 == 0, x 16-byte aligned): thread t takes the float4 k = 4 (t & 7) of rows (t >> 3) + 32 q
template <int VEC>
__device__ inline void load_chunk(const float *__restrict__ xv, int n, int d, int r0, int k0, float *v) {
    const int t = threadIdx.x;
    if constexpr (VEC == 4) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int row = r0 + (t >> 3) + 32 * q, k = k0 + 4 * (t & 7);
            f32x4 u = {0.f, 0.f, 0.f, 0.f};
            if (row < n && k < d) u = *(const f32x4 *)(xv + (size_t)row * d + k);
            v[4 * q + 0] = u[0]; v[4 * q + 1] = u[1]; v[4 * q + 2] = u[2]; v[4 * q + 3] = u[3];
        }
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int row = r0 + (t >> 5) + 8 * q, k = k0 + (t & 31);
            v[q] = (row < n && k < d) ? xv[(size_t)row * d + k] : 0.f;
        }
    }
}

template <int VEC>
__device__ inline void store_chunk(float (*L)[GLD], const float *v) {
    const int t = threadIdx.x;
    if constexpr (VEC == 4) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c) L[(t >> 3) + 32 * q][4 * (t & 7) + c] = v[4 * q + c];
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) L[(t >> 5) + 8 * q][t & 31] = v[q];
    }
}

template <int VEC>
__global__ __launch_bounds__(GNT) void kts_gram(const float *__restrict__ x, int d, const KtsGramVideo *__restrict__ vids,
                                                int B, int kind, double gamma, const double *__restrict__ nrm,
                                                char *__restrict__ kbase) {
    __shared__ float lds[2 * GT * GLD];                      // operand chunks A | B; then the transposed tile [64][65]
    static_assert(GT * TLD <= 2 * GT * GLD, "the transposed tile reuses the operand chunks");
    float (*As)[GLD] = (float (*)[GLD])lds;
    float (*Bs)[GLD] = (float (*)[GLD])(lds + GT * GLD);
    float (*Tt)[TLD] = (float (*)[TLD])lds;

    // the video of this block: the last v with tile0 <= blockIdx.x
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (vids[mid].tile0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const KtsGramVideo V = vids[lo];
    int ti, tj;
    tri_decode((int)blockIdx.x - V.tile0, ti, tj);
    const int n = V.n, i0 = ti * GT, j0 = tj * GT;
    if (i0 >= n) return;                                     // cannot happen with a consistent table; uniform per block
    const bool diag = ti == tj;
    const float *xv = x + (size_t)V.row0 * d;

    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wr = w >> 1, wc = w & 1;
    const bool idle = diag && wr == 0 && wc == 1;            // mirror of the (1, 0) quadrant
    const float (*Bop)[GLD] = diag ? As : Bs;

    f32x16 acc;
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = 0.f;

    float va[8], vb[8];
    load_chunk<VEC>(xv, n, d, i0, 0, va);
    if (!diag) load_chunk<VEC>(xv, n, d, j0, 0, vb);
    for (int k0 = 0; k0 < d; k0 += GK) {
        store_chunk<VEC>(As, va);
        if (!diag) store_chunk<VEC>(Bs, vb);
        __syncthreads();
        if (k0 + GK < d) {                                   // the next chunk's loads fly under this chunk's MFMAs
            load_chunk<VEC>(xv, n, d, i0, k0 + GK, va);
            if (!diag) load_chunk<VEC>(xv, n, d, j0, k0 + GK, vb);
        }
        if (!idle) {
#pragma unroll
            for (int kk = 0; kk < GK / 2; ++kk)
                acc = MFMA32(As[32 * wr + r][2 * kk + h], Bop[32 * wc + r][2 * kk + h], acc);
        }
        __syncthreads();
    }

    // epilogue on the accumulator; element t of lane (r, h): row i0 + 32 wr + acc_row(t, h), column j0 + 32 wc + r
    float *K = (float *)(kbase + V.k_off);
    const int ldk = V.ldk, gj = j0 + 32 * wc + r;
    const double *nv = nrm ? nrm + V.row0 : nullptr;
    const double cj = (nv && gj < n) ? nv[gj] : 0.0;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int li = 32 * wr + acc_row(t, h), gi = i0 + li;
        float v = acc[t];
        if (!idle && gi < n && gj < n && gi >= gj) {
            if (kind == 1) {                                 // cosine
                const double ci = nv[gi];
                if (gi == gj) v = ci > 0.0 ? 1.f : 0.f;
                else {
                    double c = (double)v * ci * cj;
                    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
                    v = (float)c;
                }
            } else if (kind == 2) {                          // rbf
                if (gi == gj) v = 1.f;
                else {
                    double d2 = nv[gi] + cj - 2.0 * (double)v;
                    d2 = d2 > 0.0 ? d2 : 0.0;
                    v = (float)exp(-gamma * d2);
                }
            }
            K[(size_t)gi * ldk + gj] = v;
        }
        if (!idle) Tt[32 * wc + r][li] = v;                  // transposed: [local column][local row]
    }
    __syncthreads();
    // mirror: K[j][i] for i > j, rows of 64 consecutive i
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int gi = i0 + tx;
#pragma unroll 4
    for (int q = 0; q < GT / 4; ++q) {
        const int lj = ty + 4 * q, gjm = j0 + lj;
        if (gi < n && gjm < n && gi > gjm) K[(size_t)gjm * ldk + gi] = Tt[lj][tx];
    }
}

// one thread per video: the sum, left to right, of the scatters J[b_i][b_{i+1} - 1] = W[b_{i+1}][b_i] of the segments
// that the change points c_off[0 .. m) cut - the additions of the dynamic program along that path, in its order
__global__ void kts_eval(const KtsVideo *__restrict__ vids, int B, char *__restrict__ ws) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const KtsVideo &V = vids[b];
    const int ld = V.n + 1;
    const double *W = (const double *)(ws + V.w_off);
    const int32_t *cps = (const int32_t *)(ws + V.c_off);
    int start = 0;
    double total = 0.0;
    for (int i = 0; i <= V.m; ++i) {
        const int end = i < V.m ? cps[i] : V.n;
        const double j = W[(size_t)end * ld + start];
        total = i == 0 ? j : total + j;
        start = end;
    }
    ((double *)(ws + V.s_off))[0] = total;
}

}  // namespace

#define KTS_CHECK()                                         \
    do {                                                    \
        const hipError_t e_ = hipGetLastError();            \
        if (e_ != hipSuccess) return (int)e_;               \
    } while (0)

int vsk_kts_put(const void *src, size_t bytes, void *dst, hipStream_t st) {
    const int32_t *s = (const int32_t *)src;                 // bytes is a multiple of 4 (the callers' tables are)
    size_t words = bytes / 4;
    int32_t *d = (int32_t *)dst;
    while (words) {
        const int nw = (int)(words < (size_t)KTS_BLOB_WORDS ? words : (size_t)KTS_BLOB_WORDS);
        KtsBlob blob = {};
        for (int i = 0; i < nw; ++i) blob.w[i] = s[i];
        hipLaunchKernelGGL(kts_put, dim3(1), dim3(GNT), 0, st, blob, d, nw);
        KTS_CHECK();
        s += nw; d += nw; words -= nw;
    }
    return 0;
}

int vsk_kts_row_norms(const float *x, int d, int rows, int inverse, double *out, hipStream_t st) {
    hipLaunchKernelGGL(kts_row_norms, dim3((rows + GNT / 64 - 1) / (GNT / 64)), dim3(GNT), 0, st, x, d, rows, inverse, out);
    KTS_CHECK();
    return 0;
}

int vsk_kts_gram(const float *x, int d, const KtsGramVideo *vids, int B, int tiles, int kind, double gamma,
                 const double *nrm, void *kbase, hipStream_t st) {
    if (tiles <= 0) return -1;
    const bool vec = d % 4 == 0 && ((uintptr_t)x & 15) == 0;
    if (vec) hipLaunchKernelGGL(kts_gram<4>, dim3(tiles), dim3(GNT), 0, st, x, d, vids, B, kind, gamma, nrm, (char *)kbase);
    else hipLaunchKernelGGL(kts_gram<1>, dim3(tiles), dim3(GNT), 0, st, x, d, vids, B, kind, gamma, nrm, (char *)kbase);
    KTS_CHECK();
    return 0;
}

int vsk_kts_eval(const KtsVideo *vids, int B, char *ws, hipStream_t st) {
    hipLaunchKernelGGL(kts_eval, dim3((B + 63) / 64), dim3(64), 0, st, vids, B, ws);
    KTS_CHECK();
    return 0;
}
