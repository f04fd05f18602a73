// Kernel temporal segmentation (KTS) on gfx950: the scatter table and the change-point dynamic program.
// The Gram K = X X^T runs on the existing exact-fp32 GEMM (vsk_linear); everything after it is fp64.
//
// Layout (per video, n frames, ld = n + 1):
//   W[r][c]  = K2[r][c] = sum_{a < r, b < c} K[a][b]          (r, c in [0, n]; row 0 and column 0 are zero)
//   then, in place, the strict lower triangle becomes the scatter table BY SEGMENT END:
//   W[e + 1][s] = J[s][e] = scatter of frames s..e             (s <= e)
//   The diagonal and the upper triangle keep K2: every J entry reads K2[e+1][s] (its own slot), K2[s][e+1] (upper),
//   K2[e+1][e+1] and K2[s][s] (diagonal), so no entry reads a slot another thread writes.
//   The dynamic program's step for segment end l - 1 reads row l of W contiguously beside the contiguous row I[k-1].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vs_segment_kernels.h"

namespace {

constexpr int NT = 256;                 // threads per block of the scan / table kernels (4 waves)
constexpr double KTS_BIG = 1e100;       // the reference's "nearly infinity" of a reachable-but-unset I[k, l]
constexpr double KTS_UNSET = 1e101;     // the reference's initial value of I

__device__ inline const KtsVideo &vid(const KtsVideo *v, int b) { return v[b]; }

// Exclusive prefix of v over the 256 threads of the block; `total` = the block's sum.  Uses lds[4].
__device__ inline double block_excl_scan(double v, double *lds, double &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    double ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = 0.0;
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    double off = 0.0, tot = 0.0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
        const double s = lds[i];
        if (i < w) off += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return off + ex;
}

// out[c] = sum_{b < c} x(b) for c in [0, n], x(b) = load(b) for b < n.  Whole block, uniform trip count.
template <class F>
__device__ inline void block_prefix_store(F load, double *out, int n, double *lds) {
    double carry = 0.0;
    for (int base = 0; base <= n; base += 4 * NT) {
        const int c0 = base + 4 * threadIdx.x;
        double x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = c0 + j < n ? load(c0 + j) : 0.0;
        double tot;
        double run = carry + block_excl_scan(((x[0] + x[1]) + x[2]) + x[3], lds, tot);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (c0 + j <= n) out[c0 + j] = run;
            run += x[j];
        }
        carry += tot;
    }
}

// block (r, b): r == 0 zeroes row 0 of W and writes K1 = prefix of diag(K); r >= 1 writes W[r][c] = sum_{j<c} K[r-1][j]
template <class T>
__global__ __launch_bounds__(NT) void kts_rowscan(const KtsVideo *__restrict__ vids, char *__restrict__ ws,
                                                  const char *__restrict__ kbase) {
    __shared__ double lds[NT / 64];
    const KtsVideo &V = vid(vids, blockIdx.y);
    const int r = blockIdx.x, n = V.n, ld = n + 1;
    if (r > n) return;
    const T *K = (const T *)(kbase + V.k_off);
    double *W = (double *)(ws + V.w_off);
    if (r == 0) {
        for (int c = threadIdx.x; c <= n; c += NT) W[c] = 0.0;
        const int ldk = V.ldk;
        block_prefix_store([&](int j) { return (double)K[(size_t)j * ldk + j]; }, (double *)(ws + V.k1_off), n, lds);
        return;
    }
    const T *row = K + (size_t)(r - 1) * V.ldk;
    block_prefix_store([&](int j) { return (double)row[j]; }, W + (size_t)r * ld, n, lds);
}

// column totals of the row chunk blockIdx.y (rows 1 + 64 y .. 64 y + 64) of W
__global__ __launch_bounds__(NT) void kts_colsum(const KtsVideo *__restrict__ vids, char *__restrict__ ws) {
    const KtsVideo &V = vid(vids, blockIdx.z);
    const int n = V.n, ld = n + 1, col = blockIdx.x * NT + threadIdx.x, r0 = 1 + blockIdx.y * KTS_CHUNK;
    if (col > n || r0 > n) return;
    const int r1 = min(n, r0 + KTS_CHUNK - 1);
    const double *W = (const double *)(ws + V.w_off);
    double s = 0.0;
#pragma unroll 8
    for (int r = r0; r <= r1; ++r) s += W[(size_t)r * ld + col];
    ((double *)(ws + V.t_off))[(size_t)blockIdx.y * ld + col] = s;
}

// W[r][col] = (totals of the earlier chunks) + running sum inside the chunk: the column scan that completes K2
__global__ __launch_bounds__(NT) void kts_colapply(const KtsVideo *__restrict__ vids, char *__restrict__ ws) {
    const KtsVideo &V = vid(vids, blockIdx.z);
    const int n = V.n, ld = n + 1, col = blockIdx.x * NT + threadIdx.x, r0 = 1 + blockIdx.y * KTS_CHUNK;
    if (col > n || r0 > n) return;
    const int r1 = min(n, r0 + KTS_CHUNK - 1);
    const double *Tt = (const double *)(ws + V.t_off);
    double acc = 0.0;
    for (int c = 0; c < (int)blockIdx.y; ++c) acc += Tt[(size_t)c * ld + col];
    double *W = (double *)(ws + V.w_off);
#pragma unroll 8
    for (int r = r0; r <= r1; ++r) {
        acc += W[(size_t)r * ld + col];
        W[(size_t)r * ld + col] = acc;
    }
}

// J in place, 32 x 32 tiles of (segment end e, start s), s <= e; the upper K2 tile read transposed through LDS.
// The reference's expression order: K1[e+1] - K1[s] - (K2[e+1][e+1] + K2[s][s] - K2[e+1][s] - K2[s][e+1]) / (e - s + 1).
__global__ __launch_bounds__(NT) void kts_scatter(const KtsVideo *__restrict__ vids, char *__restrict__ ws) {
#pragma clang fp contract(off)
    __shared__ double U[32][33];
    const KtsVideo &V = vid(vids, blockIdx.z);
    const int n = V.n, ld = n + 1, s0 = blockIdx.x * 32, e0 = blockIdx.y * 32;
    if (s0 > e0 || e0 >= n) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    double *W = (double *)(ws + V.w_off);
    const double *K1 = (const double *)(ws + V.k1_off);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = ty + 8 * q, s = s0 + i, e1 = e0 + 1 + tx;
        if (s < n && e1 <= n && s < e1) U[i][tx] = W[(size_t)s * ld + e1];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = e0 + ty + 8 * q, s = s0 + tx;
        if (e < n && s <= e) {
            double *slot = W + (size_t)(e + 1) * ld + s;
            const double dd = W[(size_t)(e + 1) * ld + e + 1], ds = W[(size_t)s * ld + s];
            const double num = ((dd + ds) - *slot) - U[tx][ty + 8 * q];
            *slot = (K1[e + 1] - K1[s]) - num / (double)(e - s + 1);
        }
    }
}

// I[0][l] = J[0][l-1] for lmin <= l < lmax (the reference's slice I[0, lmin:lmax]), 1e101 elsewhere
__global__ __launch_bounds__(NT) void kts_dp_init(const KtsVideo *__restrict__ vids, char *__restrict__ ws) {
    const KtsVideo &V = vid(vids, blockIdx.y);
    const int n = V.n, ld = n + 1, l = blockIdx.x * NT + threadIdx.x;
    if (l > n) return;
    const double *W = (const double *)(ws + V.w_off);
    const double v = (l >= V.lmin && l < V.lmax) ? W[(size_t)l * ld] : KTS_UNSET;
    ((double *)(ws + V.i_off))[l] = v;
    if (l == n) ((double *)(ws + V.s_off))[0] = v;
}

// Step k: one wave per segment end l, I[k][l] = min_t I[k-1][t] + J[t][l-1] over t in [max(k lmin, l - lmax), l - lmin].
// The reference keeps the first t with a strictly smaller value starting from 1e100: the minimum with ties to the
// smallest t, applied only when it is below 1e100 (else I = 1e100, p = 0).
__global__ __launch_bounds__(NT) void kts_dp_step(const KtsVideo *__restrict__ vids, char *__restrict__ ws, int k) {
    const KtsVideo &V = vid(vids, blockIdx.y);
    if (k > V.m) return;
    const int n = V.n, ld = n + 1, lane = threadIdx.x & 63;
    const int l = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (l > n) return;
    const double *Ip = (const double *)(ws + V.i_off) + (size_t)((k - 1) & 1) * ld;
    double *Ic = (double *)(ws + V.i_off) + (size_t)(k & 1) * ld;
    int32_t *P = V.p_off >= 0 ? (int32_t *)(ws + V.p_off) + (size_t)k * ld : nullptr;
    const int lmin = V.lmin;
    double out = KTS_UNSET;
    int arg = 0;
    if (l >= (k + 1) * lmin) {
        const int t0 = max(k * lmin, l - V.lmax), t1 = l - lmin;
        const double *Jr = (const double *)(ws + V.w_off) + (size_t)l * ld;       // J[t][l-1] = W[l][t]
        double best = __builtin_inf();
        int bi = 0x7fffffff;
        int t = t0 + lane;
        for (; t + 192 <= t1; t += 256) {          // four loads in flight per lane, compared in ascending t
            double c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = Ip[t + 64 * j] + Jr[t + 64 * j];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c[j] < best) { best = c[j]; bi = t + 64 * j; }
        }
        for (; t <= t1; t += 64) {
            const double c = Ip[t] + Jr[t];
            if (c < best) { best = c; bi = t; }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (best < KTS_BIG) { out = best; arg = bi; }
        else out = KTS_BIG;
    }
    if (lane == 0) {
        Ic[l] = out;
        if (P) P[l] = arg;
        if (l == n) ((double *)(ws + V.s_off))[k] = out;
    }
}

__global__ void kts_backtrack(const KtsVideo *__restrict__ vids, int B, char *__restrict__ ws) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const KtsVideo &V = vid(vids, b);
    if (V.p_off < 0) return;
    const int ld = V.n + 1;
    const int32_t *P = (const int32_t *)(ws + V.p_off);
    int32_t *cps = (int32_t *)(ws + V.c_off);
    int cur = V.n;
    for (int k = V.mbest; k >= 1; --k) {
        cur = P[(size_t)k * ld + cur];
        cps[k - 1] = cur;
    }
}

// out[i][j] = J[i][j] = W[j + 1][i] for j >= i, else 0 (tile transpose through LDS)
__global__ __launch_bounds__(NT) void kts_scatters_out(const KtsVideo *__restrict__ vids, const char *__restrict__ ws,
                                                       double *__restrict__ out) {
    __shared__ double L[32][33];
    const KtsVideo &V = vids[0];
    const int n = V.n, ld = n + 1, j0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const double *W = (const double *)(ws + V.w_off);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int jj = ty + 8 * q, j = j0 + jj, i = i0 + tx;
        L[jj][tx] = (j < n && i <= j) ? W[(size_t)(j + 1) * ld + i] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ii = ty + 8 * q, i = i0 + ii, j = j0 + tx;
        if (i < n && j < n) out[(size_t)i * n + j] = L[tx][ii];
    }
}

}  // namespace

#define KTS_CHECK()                                         \
    do {                                                    \
        const hipError_t e_ = hipGetLastError();            \
        if (e_ != hipSuccess) return (int)e_;               \
    } while (0)

int vsk_kts_scatter_table(const KtsVideo *vids, int B, int n_max, char *ws, const void *kbase, int kdouble, hipStream_t st) {
    const char *kb = (const char *)kbase;
    if (kdouble) hipLaunchKernelGGL(kts_rowscan<double>, dim3(n_max + 1, B), dim3(NT), 0, st, vids, ws, kb);
    else hipLaunchKernelGGL(kts_rowscan<float>, dim3(n_max + 1, B), dim3(NT), 0, st, vids, ws, kb);
    KTS_CHECK();
    const dim3 cgrid((n_max + NT) / NT, (n_max + KTS_CHUNK - 1) / KTS_CHUNK, B);
    hipLaunchKernelGGL(kts_colsum, cgrid, dim3(NT), 0, st, vids, ws);
    KTS_CHECK();
    hipLaunchKernelGGL(kts_colapply, cgrid, dim3(NT), 0, st, vids, ws);
    KTS_CHECK();
    const int tiles = (n_max + 31) / 32;
    hipLaunchKernelGGL(kts_scatter, dim3(tiles, tiles, B), dim3(NT), 0, st, vids, ws);
    KTS_CHECK();
    return 0;
}

int vsk_kts_dp_init(const KtsVideo *vids, int B, int n_max, char *ws, hipStream_t st) {
    hipLaunchKernelGGL(kts_dp_init, dim3((n_max + NT) / NT, B), dim3(NT), 0, st, vids, ws);
    KTS_CHECK();
    return 0;
}

int vsk_kts_dp_step(const KtsVideo *vids, int B, int n_max, int k, char *ws, hipStream_t st) {
    hipLaunchKernelGGL(kts_dp_step, dim3((n_max + NT / 64) / (NT / 64), B), dim3(NT), 0, st, vids, ws, k);
    KTS_CHECK();
    return 0;
}

int vsk_kts_backtrack(const KtsVideo *vids, int B, char *ws, hipStream_t st) {
    hipLaunchKernelGGL(kts_backtrack, dim3((B + 63) / 64), dim3(64), 0, st, vids, B, ws);
    KTS_CHECK();
    return 0;
}

int vsk_kts_scatters_out(const KtsVideo *vids, int n, const char *ws, double *out, hipStream_t st) {
    const int tiles = (n + 31) / 32;
    hipLaunchKernelGGL(kts_scatters_out, dim3(tiles, tiles), dim3(NT), 0, st, vids, ws, out);
    KTS_CHECK();
    return 0;
}
