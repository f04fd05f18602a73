/*
 * vs_summary.h — C ABI of the keyshot SUMMARY on the device: importance scores that still lie in device memory in, the
 * per-frame 0/1 summary and the list of selected frames (the content of the reference's summary.json) in device memory
 * out.  Reference: src/generate_summary_image.py:39-80 (get_summary) -> src/evaluation/generate_summary.py:17-55, per
 * video; the host path of the same work is vs_eval_generate_summary (vs_eval.h), unchanged.
 *
 * The call is stateless and needs no user annotations: the small per-call tables (a few ints per pick and per shot) are
 * staged on the host and uploaded inside the call; nothing on the host runs per frame.  Three launches for the whole
 * batch: the picks are expanded to the per-frame source table, one block per video takes the float32 shot means (numpy's
 * pairwise order), the double knapsack table and its back-track (the device functions of the device evaluation,
 * vs_eval_device.h), and a fill pass writes every frame of the summary and every selected frame's index.  The results
 * are the host path's bit for bit.
 *
 * Per video v (L_v = last_shot_end_v + 1):
 *   up-sampled value of frame f   scores[i] on [clip(positions'[i]), clip(positions'[i + 1])), positions' = positions with
 *                                 n_frames appended unless its last entry equals it, clip to [0, n_frames]; 0 for the
 *                                 segment i == n_scores and where no segment covers f; a segment i > n_scores is invalid
 *   shot s = [a, b]               weight b - a + 1 (unclipped, >= 0); value the float32 mean over the frames
 *                                 [lo, hi) = [max(0, min(a, n_frames)), max(lo, min(b + 1, n_frames))), NaN when empty
 *   budget                        W = (int)((double)L_v * proportion)
 *   selection                     knapsack_implementation.py, table in double, Python's max() with NaNs, back-track on
 *                                 K[i][w] != K[i-1][w]; a capacity walked below -(W + 1) fails the call (IndexError)
 *   summary                       int8 [L_v], 1 on [max(0, a), min(L_v - 1, b)] of every selected shot
 *
 * Preconditions, checked on the host before any device call (VS_ERR_INVALID): n_shots >= 1, n_positions >= 1,
 * 0 <= n_frames <= 2^18, n_scores >= 0, positions non-decreasing (the segments are then disjoint), 0 <= last_shot_end <
 * 2^24, the shots clipped to [0, last_shot_end] ascending and disjoint, proportion finite and in [0, 1], n_videos <=
 * 65535.  Scores must be finite (as for the device evaluation).
 *
 * Every function returns 0 or a VS_ERR_* status (vs_scorer.h) and sets vs_last_error().
 */
#ifndef VS_SUMMARY_H
#define VS_SUMMARY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device workspace vs_summarize needs for these videos; 0 on invalid arguments (vs_last_error() says why).
 * All pointers are HOST pointers: n_positions, n_frames, n_shots [n_videos]; change_points [sum n_shots][2]. */
size_t vs_summarize_workspace_bytes(int32_t n_videos, const int32_t *n_positions, const int32_t *n_frames,
                                    const int32_t *n_shots, const int32_t *change_points, double proportion);

/* HOST in:    n_scores, n_positions, n_frames, n_shots [n_videos]; positions [sum n_positions] (the videos' picks
 *             concatenated); change_points [sum n_shots][2], inclusive ends (the format of vs_eval_generate_summary);
 *             proportion (the reference's 0.15).
 * DEVICE in:  scores_dev float [sum n_scores], concatenated in video order.
 * DEVICE out: summary_dev int8 [sum L_v], video v at offset sum_{u<v} L_u; frames_dev int32, same offsets and capacity:
 *             the first n_selected_frames[v] entries of video v's slice are the ascending frame indices where its
 *             summary is 1, the rest of the slice is not written.
 * HOST out:   n_selected_frames [n_videos]; selected_shots_or_null int8 [sum n_shots] (1 where the knapsack took the
 *             shot); shot_means_or_null double [sum n_shots] (the float32 means, widened).
 * workspace:  DEVICE, at least vs_summarize_workspace_bytes(...) bytes, 256-byte aligned.
 * Synchronises `stream` before it returns. */
int vs_summarize(int32_t n_videos, const int32_t *n_scores, const int32_t *n_positions, const int32_t *n_frames,
                 const int32_t *n_shots, const int32_t *positions, const int32_t *change_points, double proportion,
                 const float *scores_dev, int8_t *summary_dev, int32_t *frames_dev, int32_t *n_selected_frames,
                 int8_t *selected_shots_or_null, double *shot_means_or_null, void *workspace, size_t workspace_bytes,
                 void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VS_SUMMARY_H */
