// Internal interface between the device evaluation's C ABI (vs_eval_device.cpp) and its kernels (vs_eval_device.hip).
// Every launcher enqueues on `st`, never synchronises, and returns 0 or a hipError_t.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- static per set (built on the host at creation, uploaded once) ----
// One video.  Every *_off is an ELEMENT index into the flat array named beside it.
struct EvVideo {
    int32_t n_frames, n_shots, n_users, n_score_users, n_scores, n_xruns;
    int32_t W;                // knapsack budget int((last_shot_end + 1) * 0.15), taken in double on the host
    int32_t reserved;
    int64_t frame_off;        // frame_src  [n_frames]
    int64_t shot_off;         // shot_lo / shot_hi / shot_wt / shot_clip  [n_shots]
    int64_t cnt_off;          // cnt  [n_users][n_shots]
    int64_t xrun_off;         // xrun_src / xrun_w  [n_xruns]
    int64_t pair_off;         // pairs  [n_score_users]
};
// One (video, user) of the rank correlation: its joint runs of pick runs and user runs.
struct EvPair {
    int64_t j_off;            // jw / jx / jy  [m]
    int32_t m, reserved;
};
struct EvStatic {
    const EvVideo *vid;
    const int32_t *frame_src;             // per frame: the pick whose score the up-sampled vector holds there, or -1 (value 0)
    const int32_t *shot_lo, *shot_hi;     // frames [lo, hi) the shot's mean runs over (clipped to n_frames; empty: NaN)
    const int32_t *shot_wt;               // the knapsack weight: the shot's unclipped length
    const int32_t *shot_clip;             // frames the shot sets in the summary
    const int32_t *cnt;                   // per (user, shot): frames of the user's summary inside the shot
    const int32_t *xrun_src, *xrun_w;     // runs of frame_src: pick (or -1) and length
    const EvPair *pairs;
    const int32_t *jw, *jx, *jy;          // joint run: frames, x run (index into the video's xruns), the user's DOUBLED average rank
};

// ---- per run (laid out in the caller's workspace) ----
struct EvSlot {
    int32_t video;
    int32_t score_off;        // this video's first score in scores_dev
    int32_t shot_out;         // sel / val  [n_shots]
    int32_t user_out;         // ov  [n_users]
    int32_t xrun_out;         // rank2x  [n_xruns]
    int32_t pair_out;         // pairout  [n_score_users]
    int64_t bits_off;         // bits  [n_shots][ceil((W + 1) / 64)] uint64
    int64_t rows_off;         // rows  [2][W + 1] doubles when the two live knapsack rows do not fit in LDS, else -1
};
struct EvTask { int32_t slot, user; };
struct EvRun {
    const EvSlot *slots;
    const EvTask *tasks;
    const float *scores;
    int64_t *vidout;          // [n_slots][4]: sumS, error flag, 2 * xtie, 4 * saa
    int64_t *pairout;         // [n_pairs][3]: dis, ntie, 4 * sab
    int32_t *ov;              // per (slot, user): overlap of the selection and the user's summary
    int8_t *sel;              // per (slot, shot): taken by the knapsack
    double *val;              // per (slot, shot): the shot's mean
    int32_t *rank2x;          // per (slot, x run): the DOUBLED average rank of its value
    unsigned long long *bits; // K[i][w] != K[i-1][w]
    double *rows;
};

enum { EV_NT = 256,           // threads per block; also the knapsack's columns per pass
       EV_LDS_COLS = 2048,    // knapsack rows of up to this many columns (W + 1) live in LDS (2 x 16 KiB)
       EV_LDS_BITS = 3072 };  // ... and the change bits of up to this many 64-bit words (24 KiB), else in the workspace

int vsk_eval_summary(const EvStatic &S, const EvRun &R, int n_slots, hipStream_t st);
int vsk_eval_xrank(const EvStatic &S, const EvRun &R, int n_slots, hipStream_t st);
int vsk_eval_pairs(const EvStatic &S, const EvRun &R, int n_tasks, hipStream_t st);
