// Internal interface between the device summary's C ABI (vs_summary.cpp) and its kernels (vs_summary.hip).
// Every launcher enqueues on `st`, never synchronises, and returns 0 or a hipError_t.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One video of a call.  Every *_off is an ELEMENT index into the flat array named beside it.
struct SmVideo {
    int32_t n_frames, n_shots;
    int32_t n_ne;             // shots that set at least one frame of the summary
    int32_t W;                // knapsack budget int(L * proportion), taken in double on the host
    int32_t L;                // frames of the summary: last_shot_end + 1
    int32_t reserved;
    int64_t score_off;        // scores  [n_scores]
    int64_t frame_off;        // frame_src  [n_frames]
    int64_t shot_off;         // shot_lo / shot_hi / shot_wt / shot_clip / shot_dst / sel / val  [n_shots]
    int64_t ne_off;           // ne_start / ne_end / ne_shot  [n_ne]
    int64_t out_off;          // summary / frames  [L]
    int64_t bits_off;         // bits  [n_shots][ceil((W + 1) / 64)] uint64
    int64_t rows_off;         // rows  [2][W + 1] doubles when the two live knapsack rows do not fit in LDS, else -1
};
// One pick segment: frames [lo, hi) of a video take the score `src` (-1: the value 0).
struct SmSeg {
    int64_t base;             // the video's frame_off
    int32_t lo, hi, src, reserved;
};
struct SmArgs {
    const SmVideo *vid;
    const SmSeg *seg;
    int64_t n_seg;
    const int32_t *shot_lo, *shot_hi;     // frames [lo, hi) the shot's mean runs over (clipped to n_frames; empty: NaN)
    const int32_t *shot_wt;               // the knapsack weight: the shot's unclipped length
    const int32_t *shot_clip;             // frames the shot sets in the summary
    const int32_t *ne_start, *ne_end;     // the non-empty shots' frames [start, end] in the summary, ascending and disjoint
    const int32_t *ne_shot;               // ... and their shot index
    const float *scores;
    int32_t *frame_src;       // per frame: the pick whose score the up-sampled vector holds there, or -1 (value 0)
    int32_t *shot_dst;        // per shot: offset of its first frame in the video's slice of `frames`, -1 when not selected
    int64_t *vidout;          // [n_videos][2]: selected frames, error flag
    double *val;              // per shot: its mean
    int8_t *sel;              // per shot: taken by the knapsack
    unsigned long long *bits; // K[i][w] != K[i-1][w]
    double *rows;
    int8_t *summary;
    int32_t *frames;
};

enum { SM_NT = 256,           // threads per block of the three kernels
       SM_FILL_TILE = 1024 }; // summary bytes per block of summary_fill: four per lane, one 32-bit store

int vsk_summary_expand_picks(const SmArgs &A, hipStream_t st);
int vsk_summary_select(const SmArgs &A, int n_videos, hipStream_t st);
int vsk_summary_fill(const SmArgs &A, int n_videos, int max_L, hipStream_t st);
