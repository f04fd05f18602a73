/*
 * vs_eval_device.h — C ABI of the keyshot evaluation ON THE DEVICE (opt-in; the host path of vs_eval.h is unchanged).
 * Same work as vs_eval_corpus (reference src/evaluation/compute_metrics.py:42 eval_metrics, per video), from scores that
 * still lie in device memory where the scorer wrote them.
 *
 * Split: everything that does not depend on the scores is computed ONCE, on the host, when the set is created (clipped
 * pick boundaries, shot ranges and lengths, the knapsack budget, the users' summaries counted per shot, the users'
 * run-compressed importance scores with their ranks and tie counts, the joint runs of picks and user runs) and uploaded
 * once.  A run computes, per video, the float32 shot means (numpy's pairwise order), the double knapsack table and its
 * back-track, the prediction's ranks, and per (video, user) the pair counts; what comes back per (video, user) is exact
 * integers, and the last few double operations (precision / recall / F, tau-b, rho) run on the host with the expressions
 * of the host path.  The results are therefore the host path's bit for bit.
 *
 * Preconditions beyond vs_eval_corpus's: every score is FINITE (the host path orders NaNs by position; the device path
 * does not reproduce that); the shots of a video, clipped to [0, last_shot_end], are ascending and disjoint (as any
 * segmentation's are); n_frames <= 2^18 (the Spearman sums
 * stay exact in double as well as in int64).  Records that break the last two are rejected at creation.
 *
 * Every function returns 0 or a VS_ERR_* status (vs_scorer.h) and sets vs_last_error().
 */
#ifndef VS_EVAL_DEVICE_H
#define VS_EVAL_DEVICE_H

#include <stddef.h>
#include <stdint.h>

#include "vs_eval.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vs_eval_set vs_eval_set;

/* Builds the static part for `videos` (the records of vs_eval_corpus: HOST pointers; `scores` may be NULL, n_scores
 * counts the scores a run will bring for that video) and uploads it on `stream` (synchronised before return).
 * Argument checks come first and need no GPU; on a host without a device the set is still built, and the first run
 * uploads it.  A record the host path would reject for its shape (a shot of negative
 * length, more pick segments than n_scores + 1) is rejected here. */
int vs_eval_set_create(const vs_eval_video *videos, int32_t n_videos, void *stream, vs_eval_set **out);

void vs_eval_set_free(vs_eval_set *set);

/* Bytes of device workspace a run over these videos needs; 0 on invalid arguments (vs_last_error() says why). */
size_t vs_eval_set_workspace_bytes(const vs_eval_set *set, const int32_t *video_ids, int32_t n_ids);

/* Evaluates the videos video_ids[0 .. n_ids) (indices into the set; repeats allowed).
 * scores_dev: DEVICE float, the listed videos' n_scores scores each, concatenated in video_ids order.
 * f_score, kendall, spearman: HOST out [n_ids] (kendall / spearman NaN for a video without user_scores).
 * selected_or_null: HOST out [sum of the listed videos' n_shots], 1 where the knapsack took the shot; or NULL.
 * workspace: DEVICE, at least vs_eval_set_workspace_bytes(...) bytes, 256-byte aligned.
 * Synchronises `stream` before it returns.  A video whose back-track walks the capacity below -(W + 1) (IndexError in
 * the reference, reachable through NaN shot means) fails the call with VS_ERR_INVALID, as the host path does. */
int vs_eval_set_run(vs_eval_set *set, const float *scores_dev, const int32_t *video_ids, int32_t n_ids,
                    double *f_score, double *kendall, double *spearman, int8_t *selected_or_null,
                    void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VS_EVAL_DEVICE_H */
