// vs_summary.hip — kernels of the keyshot summary on the device (include/vs_summary.h).
// Three launches per call over the whole batch, no atomics, no read-modify-write of an output:
//   summary_expand_picks  one wave per pick segment:   the video's frame_src table (pick index or -1), every frame once
//   summary_select        one block per video:         shot means, knapsack rows, back-track (vs_keyshot_device.h, shared with
//                                                      eval_summary), then an exclusive scan of the selected shots' clipped
//                                                      lengths: each selected shot's offset into `frames`, the video's count
//   summary_fill          grid over (frame tile, video): every frame of [0, L) gets its 0 or 1 - four frames per lane in one
//                                                      aligned 32-bit store - and every selected frame its slot in `frames`
// The shot means and the knapsack table are the reference's own float32 / double operations in the reference's order: this
// file must never be built with fast-math, contraction or reassociation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vs_device.h"
#include "vs_keyshot_device.h"
#include "vs_summary_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = SM_NT;
static_assert(SM_NT == EV_NT, "the shared device functions run with EV_NT threads per block");
static_assert(SM_FILL_TILE == 4 * SM_NT, "summary_fill: four summary bytes per lane");

__global__ __launch_bounds__(SM_NT) void summary_expand_picks(SmArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (s >= A.n_seg) return;
    const SmSeg g = A.seg[s];
    int32_t *dst = A.frame_src + g.base;
    for (int f = g.lo + lane; f < g.hi; f += 64) dst[f] = g.src;      // consecutive lanes, consecutive frames
}

__global__ __launch_bounds__(SM_NT) void summary_select(SmArgs A) {
    __shared__ double lds_rows[2 * EV_LDS_COLS];
    __shared__ unsigned long long lds_bits[EV_LDS_BITS];
    __shared__ int scan[NT];
    const SmVideo V = A.vid[blockIdx.x];
    const int t = threadIdx.x;
    const int n = V.n_shots, W = V.W;
    const float *sc = A.scores + V.score_off;
    const int32_t *src = A.frame_src + V.frame_off;
    const int32_t *lo = A.shot_lo + V.shot_off, *hi = A.shot_hi + V.shot_off, *wt = A.shot_wt + V.shot_off;
    const int32_t *clip = A.shot_clip + V.shot_off;
    double *val = A.val + V.shot_off;
    int8_t *sel = A.sel + V.shot_off;

    vs_keyshot::shot_means(src, sc, lo, hi, n, val, sel);
    double *prev = V.rows_off >= 0 ? A.rows + V.rows_off : lds_rows;
    double *cur = prev + (V.rows_off >= 0 ? W + 1 : EV_LDS_COLS);
    const int wpr = (W + 64) / 64;                            // 64-bit words of change bits per row
    unsigned long long *bits = (long long)n * wpr <= EV_LDS_BITS ? lds_bits : A.bits + V.bits_off;      // read back by ONE thread
    vs_keyshot::knapsack_rows(prev, cur, bits, wpr, wt, val, n, W);
    if (t == 0) {
        long long total = 0;
        A.vidout[2 * (size_t)blockIdx.x + 1] = vs_keyshot::backtrack(bits, wpr, wt, clip, n, W, sel, &total);
    }
    __syncthreads();

    // exclusive scan of the selected shots' clipped lengths, NT shots per pass (inclusive Hillis-Steele in LDS, then
    // minus the own length); `carry` is the same in every thread
    int32_t *dst = A.shot_dst + V.shot_off;
    int carry = 0;
    for (int s0 = 0; s0 < n; s0 += NT) {
        const int s = s0 + t;
        const bool taken = s < n && sel[s] != 0;
        const int c = taken ? clip[s] : 0;
        scan[t] = c;
        __syncthreads();
        for (int d = 1; d < NT; d <<= 1) {
            const int below = t >= d ? scan[t - d] : 0;
            __syncthreads();
            scan[t] += below;
            __syncthreads();
        }
        if (s < n) dst[s] = taken ? carry + scan[t] - c : -1;
        carry += scan[NT - 1];
        __syncthreads();                                       // scan[NT - 1] is read before the next pass overwrites it
    }
    if (t == 0) A.vidout[2 * (size_t)blockIdx.x + 0] = carry;
}

// The summary's slice of a video starts at any byte: lane k of block x owns the four bytes of the 32-bit word k of tile x,
// counted from the aligned address at or below the slice's start.  A word that lies inside the slice is one store, the (at
// most two) words across its ends are written byte by byte - never a byte of a neighbouring slice.
__global__ __launch_bounds__(SM_NT) void summary_fill(SmArgs A) {
    const SmVideo V = A.vid[blockIdx.y];
    int8_t *out = A.summary + V.out_off;
    const int mis = (int)((uintptr_t)out & 3);
    const int f0 = (int)blockIdx.x * SM_FILL_TILE + 4 * (int)threadIdx.x - mis;    // L < 2^24: no overflow
    if (f0 >= V.L) return;
    const int32_t *ns = A.ne_start + V.ne_off, *ne = A.ne_end + V.ne_off, *nshot = A.ne_shot + V.ne_off;
    const int32_t *dst = A.shot_dst + V.shot_off;
    int32_t *frames = A.frames + V.out_off;
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int f = f0 + k;
        if (f < 0 || f >= V.L) continue;
        int a = 0, b = V.n_ne;                                 // the last non-empty shot that starts at or before f
        while (a < b) {
            const int m = (a + b) >> 1;
            if (ns[m] <= f) a = m + 1; else b = m;
        }
        const int q = a - 1;
        if (q < 0 || f > ne[q]) continue;
        const int d = dst[nshot[q]];
        if (d < 0) continue;
        word |= 1u << (8 * k);
        frames[d + (f - ns[q])] = f;
    }
    if (f0 >= 0 && f0 + 3 < V.L) {
        *reinterpret_cast<uint32_t *>(out + f0) = word;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (f0 + k >= 0 && f0 + k < V.L) out[f0 + k] = (int8_t)((word >> (8 * k)) & 1u);
    }
}

}  // namespace

int vsk_summary_expand_picks(const SmArgs &A, hipStream_t st) {
    if (A.n_seg == 0) return 0;
    hipLaunchKernelGGL(summary_expand_picks, dim3((unsigned)((A.n_seg + NT / 64 - 1) / (NT / 64))), dim3(NT), 0, st, A);
    VSK_CHECK_LAUNCH();
    return 0;
}

int vsk_summary_select(const SmArgs &A, int n_videos, hipStream_t st) {
    hipLaunchKernelGGL(summary_select, dim3(n_videos), dim3(NT), 0, st, A);
    VSK_CHECK_LAUNCH();
    return 0;
}

int vsk_summary_fill(const SmArgs &A, int n_videos, int max_L, hipStream_t st) {
    hipLaunchKernelGGL(summary_fill, dim3((unsigned)((max_L + 3 + SM_FILL_TILE - 1) / SM_FILL_TILE), n_videos), dim3(NT), 0, st, A);
    VSK_CHECK_LAUNCH();
    return 0;
}
