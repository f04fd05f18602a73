// vs_keyshot_device.h — device functions of the keyshot selection, shared by the device evaluation (vs_eval_device.hip:
// eval_summary) and the device summary (vs_summary.hip: summary_select): the float32 shot mean in numpy's pairwise order,
// the double knapsack table row by row with only its change bits kept, and the back-track.  One definition, so the two
// kernels select the same shots bit for bit.
// Everything here is the reference's own float32 / double operation in the reference's order: a file that includes this
// header must never be built with fast-math, contraction or reassociation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vs_eval_device_kernels.h"

#pragma clang fp contract(off)

namespace vs_keyshot {

constexpr int NT = EV_NT;

// frame f of the up-sampled prediction: the score of the pick that covers it, 0 past the last score
__device__ __forceinline__ float frame_value(const int32_t *src, const float *sc, int f) {
    const int p = src[f];
    return p >= 0 ? sc[p] : 0.f;
}

// numpy's pairwise_sum below its recursion: n < 8 plain, n <= 128 eight strided partial sums.  EIGHT LANES (g = 0..7,
// consecutive, all with the same arguments and so the same control flow) share the call: lane g carries partial sum g,
// the eight are combined in numpy's order and every lane returns the same bits.
__device__ inline float pairwise_leaf(const int32_t *src, const float *sc, int n, int g) {
    if (n < 8) {
        float res = 0.f;
        for (int i = 0; i < n; ++i) res += frame_value(src, sc, i);
        return res;
    }
    float r = frame_value(src, sc, g);
    const int full = n - (n % 8);
    int i;
#pragma unroll 4
    for (i = 8; i < full; i += 8) r += frame_value(src, sc, i + g);
    const float r0 = __shfl(r, 0, 8), r1 = __shfl(r, 1, 8), r2 = __shfl(r, 2, 8), r3 = __shfl(r, 3, 8),
                r4 = __shfl(r, 4, 8), r5 = __shfl(r, 5, 8), r6 = __shfl(r, 6, 8), r7 = __shfl(r, 7, 8);
    float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += frame_value(src, sc, i);
    return res;
}

// np_pairwise_sum_f32 (vs_eval.cpp) without recursion: post-order walk of the same split tree (n2 = n / 2 rounded down
// to a multiple of 8), by the same eight lanes as pairwise_leaf.  n <= 2^18 frames: at most 12 levels above the leaves.
__device__ inline float pairwise_sum(const int32_t *src, const float *sc, int n, int g) {
    if (n <= 128) return pairwise_leaf(src, sc, n, g);
    int off[40], len[40];
    bool seen[40];
    float val[24];
    int top = 0, vt = 0;
    off[0] = 0; len[0] = n; seen[0] = false; top = 1;
    while (top > 0) {
        const int o = off[top - 1], l = len[top - 1];
        if (l <= 128) {
            --top;
            val[vt++] = pairwise_leaf(src + o, sc, l, g);
        } else if (seen[top - 1]) {
            --top;
            const float right = val[--vt], left = val[--vt];
            val[vt++] = left + right;
        } else {
            seen[top - 1] = true;
            int n2 = l / 2;
            n2 -= n2 % 8;
            off[top] = o + n2; len[top] = l - n2; seen[top] = false; ++top;     // right: walked second
            off[top] = o;      len[top] = n2;     seen[top] = false; ++top;     // left: walked first
        }
    }
    return val[0];
}

// shot means of one video by the whole block (NT threads), eight lanes per shot: float32 pairwise sum, float32 correctly
// rounded divide, NaN for an empty shot (generate_summary.py:42).  Writes val[s] (widened) and clears sel[s].
__device__ inline void shot_means(const int32_t *src, const float *sc, const int32_t *lo, const int32_t *hi, int n, double *val,
                                  int8_t *sel) {
    const int t = threadIdx.x;
    for (int s = t >> 3; s < n; s += NT / 8) {
        const int a = lo[s], cnt = hi[s] - a;
        const float m = cnt > 0 ? __fdiv_rn(pairwise_sum(src + a, sc, cnt, t & 7), (float)cnt) : __builtin_nanf("");
        if ((t & 7) == 0) { val[s] = (double)m; sel[s] = 0; }
    }
}

// knapsack rows (knapsack_implementation.py:11-21) by the whole block: parallel over w, rows in sequence.  prev / cur: two
// rows of W + 1 doubles (LDS or global); bits: [n][wpr] words of K[i][w] != K[i-1][w], wpr = (W + 64) / 64.  val is read
// after a barrier, so it may have been written by other threads of the block just before the call.
__device__ inline void knapsack_rows(double *prev, double *cur, unsigned long long *bits, int wpr, const int32_t *wt, const double *val,
                                     int n, int W) {
    const int t = threadIdx.x;
    for (int w = t; w <= W; w += NT) prev[w] = 0.0;
    __syncthreads();
    for (int i = 1; i <= n; ++i) {
        const int w_i = wt[i - 1];
        const double v_i = val[i - 1];
        for (int base = 0; base <= W; base += NT) {           // uniform trip count: every lane takes part in the ballot
            const int w = base + t;
            bool changed = false;
            if (w <= W) {
                double c = 0.0;                               // column 0 stays 0
                if (w >= 1) {
                    const double p = prev[w];
                    if (w_i <= w) {
                        const double take = v_i + prev[w - w_i];
                        c = p > take ? p : take;              // Python max(a, b): a unless b > a, also with a NaN on either side
                    } else {
                        c = p;
                    }
                    changed = c != p;                         // a NaN differs from everything, itself included
                }
                cur[w] = c;
            }
            const unsigned long long mask = __ballot(changed);
            const int word = (base >> 6) + (t >> 6);
            if ((t & 63) == 0 && word < wpr) bits[(size_t)(i - 1) * wpr + word] = mask;
        }
        __syncthreads();
        double *x = prev; prev = cur; cur = x;
    }
}

// back-track (:23-28), ONE thread: a "taken" shot that does not fit carries a NEGATIVE capacity on, which indexes the
// row from its end (Python list semantics) and below -(W + 1) is the reference's IndexError (returns 1).  Sets sel[s] of
// the taken shots and adds their clip[s] (the frames they set in the summary) into *sum_clip.
__device__ inline long long backtrack(const unsigned long long *bits, int wpr, const int32_t *wt, const int32_t *clip, int n, int W,
                                      int8_t *sel, long long *sum_clip) {
    long long sumS = 0, err = 0;
    int w = W;
    for (int i = n; i > 0; --i) {
        if (w < -(W + 1)) { err = 1; break; }
        const int col = w < 0 ? w + W + 1 : w;
        if ((bits[(size_t)(i - 1) * wpr + (col >> 6)] >> (col & 63)) & 1ull) {
            sel[i - 1] = 1;
            sumS += clip[i - 1];
            w -= wt[i - 1];
        }
    }
    *sum_clip = sumS;
    return err;
}

}  // namespace vs_keyshot
