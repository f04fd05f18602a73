// vs_eval_device.hip — kernels of the keyshot evaluation on the device (include/vs_eval_device.h).
// Three launches per run over the whole batch, no atomics (integer sums are order-free):
//   eval_summary  one block per video:      float32 shot means in numpy's pairwise order, the double knapsack table row by
//                                           row (only the bits K[i][w] != K[i-1][w] are kept), back-track, sumS, overlaps
//                                           (the device functions live in vs_keyshot_device.h: the device summary shares them)
//   eval_xrank    one block per video:      doubled average ranks of the pick runs, 2 * xtie, 4 * saa (weighted all-pairs counts)
//   eval_pairs    one block per (video, user): dis, ntie, 4 * sab over the joint runs - the one O(m^2) kernel
// Everything a result depends on is an exact integer or (shot means, knapsack table) the reference's own float32 / double
// operations in the reference's order: this file must never be built with fast-math, contraction or reassociation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vs_device.h"
#include "vs_eval_device_kernels.h"
#include "vs_keyshot_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = EV_NT;

// sum of one int64 per thread over the block; the result is valid in thread 0.  buf: NT entries of LDS.
__device__ long long block_sum(long long v, long long *buf) {
    const int t = threadIdx.x;
    __syncthreads();
    buf[t] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) buf[t] += buf[t + s];
        __syncthreads();
    }
    return buf[0];
}

__global__ __launch_bounds__(EV_NT) void eval_summary(EvStatic S, EvRun R) {
    __shared__ double lds_rows[2 * EV_LDS_COLS];
    __shared__ unsigned long long lds_bits[EV_LDS_BITS];
    const EvSlot sl = R.slots[blockIdx.x];
    const EvVideo V = S.vid[sl.video];
    const int t = threadIdx.x;
    const int n = V.n_shots, W = V.W;
    const float *sc = R.scores + sl.score_off;
    const int32_t *src = S.frame_src + V.frame_off;
    const int32_t *lo = S.shot_lo + V.shot_off, *hi = S.shot_hi + V.shot_off, *wt = S.shot_wt + V.shot_off;
    double *val = R.val + sl.shot_out;
    int8_t *sel = R.sel + sl.shot_out;

    // shot means, knapsack rows and back-track: the device functions shared with the device summary (vs_keyshot_device.h)
    vs_keyshot::shot_means(src, sc, lo, hi, n, val, sel);
    double *prev = sl.rows_off >= 0 ? R.rows + sl.rows_off : lds_rows;
    double *cur = prev + (sl.rows_off >= 0 ? W + 1 : EV_LDS_COLS);
    const int wpr = (W + 64) / 64;                            // 64-bit words of change bits per row
    unsigned long long *bits = (long long)n * wpr <= EV_LDS_BITS ? lds_bits : R.bits + sl.bits_off;     // read back by ONE thread
    vs_keyshot::knapsack_rows(prev, cur, bits, wpr, wt, val, n, W);
    if (t == 0) {
        long long sumS = 0;
        const long long err = vs_keyshot::backtrack(bits, wpr, wt, S.shot_clip + V.shot_off, n, W, sel, &sumS);
        R.vidout[4 * (size_t)blockIdx.x + 0] = sumS;
        R.vidout[4 * (size_t)blockIdx.x + 1] = err;
    }
    __syncthreads();

    // overlap with each user's summary from the static per-shot counts
    const int32_t *cnt = S.cnt + V.cnt_off;
    for (int u = t; u < V.n_users; u += NT) {
        int ov = 0;
        for (int s = 0; s < n; ++s) ov += sel[s] ? cnt[(size_t)u * n + s] : 0;
        R.ov[sl.user_out + u] = ov;
    }
}

// rank2x[a] = 2 * (frames with a greater value) + (frames with an equal value) + 1: twice the average rank of
// scipy.stats.rankdata(-x).  Sums of weights stay below n_frames <= 2^18: int32 inside, int64 across.
__global__ __launch_bounds__(EV_NT) void eval_xrank(EvStatic S, EvRun R) {
    __shared__ float tx[NT];
    __shared__ int tw[NT];
    __shared__ long long red[NT];
    const EvSlot sl = R.slots[blockIdx.x];
    const EvVideo V = S.vid[sl.video];
    const int t = threadIdx.x, m = V.n_xruns;
    const float *sc = R.scores + sl.score_off;
    const int32_t *xs = S.xrun_src + V.xrun_off, *xw = S.xrun_w + V.xrun_off;
    long long xtie2 = 0, saa4 = 0;
    for (int a0 = 0; a0 < m; a0 += NT) {
        const int a = a0 + t;
        float xa = 0.f;
        int wa = 0;
        if (a < m) { const int p = xs[a]; xa = p >= 0 ? sc[p] : 0.f; wa = xw[a]; }
        int gt = 0, eq = 0;
        for (int b0 = 0; b0 < m; b0 += NT) {
            __syncthreads();
            if (b0 + t < m) { const int p = xs[b0 + t]; tx[t] = p >= 0 ? sc[p] : 0.f; tw[t] = xw[b0 + t]; }
            __syncthreads();
            const int nb = min(NT, m - b0);
            for (int j = 0; j < nb; ++j) {
                const float xb = tx[j];
                const int wb = tw[j];
                gt += xb > xa ? wb : 0;
                eq += xb == xa ? wb : 0;
            }
        }
        if (a < m) {
            const int r2 = 2 * gt + eq + 1;
            R.rank2x[sl.xrun_out + a] = r2;
            const long long d = (long long)r2 - (V.n_frames + 1);
            xtie2 += (long long)wa * (eq - 1);
            saa4 += (long long)wa * d * d;
        }
    }
    xtie2 = block_sum(xtie2, red);
    saa4 = block_sum(saa4, red);
    if (t == 0) {
        R.vidout[4 * (size_t)blockIdx.x + 2] = xtie2;
        R.vidout[4 * (size_t)blockIdx.x + 3] = saa4;
    }
}

// dis = sum_{a<b} w_a w_b [(x_a - x_b)(y_a - y_b) < 0], ntie = sum_a C(w_a, 2) + sum_{a<b} w_a w_b [x_a = x_b and y_a = y_b],
// 4 sab = sum_a w_a (2 rx_a - (n + 1)) (2 ry_a - (n + 1)); x and y enter as their doubled average ranks (monotone in the values).
__global__ __launch_bounds__(EV_NT) void eval_pairs(EvStatic S, EvRun R) {
    __shared__ int tw[NT], tkx[NT], tky[NT];
    __shared__ long long red[NT];
    const EvTask task = R.tasks[blockIdx.x];
    const EvSlot sl = R.slots[task.slot];
    const EvVideo V = S.vid[sl.video];
    const EvPair P = S.pairs[V.pair_off + task.user];
    const int t = threadIdx.x, m = P.m;
    const int32_t *jw = S.jw + P.j_off, *jx = S.jx + P.j_off, *jy = S.jy + P.j_off;
    const int32_t *r2x = R.rank2x + sl.xrun_out;
    const int n1 = V.n_frames + 1;
    long long dis = 0, ntie = 0, sab4 = 0;
    for (int a0 = 0; a0 < m; a0 += NT) {
        const int a = a0 + t;
        int wa = 0, kxa = 0, kya = 0;
        if (a < m) { wa = jw[a]; kxa = r2x[jx[a]]; kya = jy[a]; }
        int accd = 0, acct = 0;
        for (int b0 = a0; b0 < m; b0 += NT) {                 // pairs a < b only: tiles from a's own onwards
            __syncthreads();
            if (b0 + t < m) { tw[t] = jw[b0 + t]; tkx[t] = r2x[jx[b0 + t]]; tky[t] = jy[b0 + t]; }
            __syncthreads();
            const int nb = min(NT, m - b0);
            for (int j = (b0 == a0 ? t + 1 : 0); j < nb; ++j) {
                const int dx = kxa - tkx[j], dy = kya - tky[j], wb = tw[j];
                accd += (dx != 0 && dy != 0 && ((dx ^ dy) < 0)) ? wb : 0;
                acct += (dx == 0 && dy == 0) ? wb : 0;
            }
        }
        if (a < m) {
            dis += (long long)wa * accd;
            ntie += (long long)wa * acct + (long long)wa * (wa - 1) / 2;
            sab4 += (long long)wa * (long long)(kxa - n1) * (long long)(kya - n1);
        }
    }
    dis = block_sum(dis, red);
    ntie = block_sum(ntie, red);
    sab4 = block_sum(sab4, red);
    if (t == 0) {
        int64_t *o = R.pairout + 3 * ((size_t)sl.pair_out + task.user);
        o[0] = dis; o[1] = ntie; o[2] = sab4;
    }
}

}  // namespace

int vsk_eval_summary(const EvStatic &S, const EvRun &R, int n_slots, hipStream_t st) {
    hipLaunchKernelGGL(eval_summary, dim3(n_slots), dim3(NT), 0, st, S, R);
    VSK_CHECK_LAUNCH();
    return 0;
}

int vsk_eval_xrank(const EvStatic &S, const EvRun &R, int n_slots, hipStream_t st) {
    hipLaunchKernelGGL(eval_xrank, dim3(n_slots), dim3(NT), 0, st, S, R);
    VSK_CHECK_LAUNCH();
    return 0;
}

int vsk_eval_pairs(const EvStatic &S, const EvRun &R, int n_tasks, hipStream_t st) {
    if (n_tasks == 0) return 0;
    hipLaunchKernelGGL(eval_pairs, dim3(n_tasks), dim3(NT), 0, st, S, R);
    VSK_CHECK_LAUNCH();
    return 0;
}
