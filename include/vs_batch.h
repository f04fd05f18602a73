/*
 * vs_batch.h — C ABI of the training INPUT on the device: a training set that was uploaded once (the videos' feature rows
 * concatenated into one arena, a per-row side array such as the targets, the row offsets of the videos) is cut into the
 * batches of an epoch by one launch per batch, with nothing crossing the host link inside the epoch.  Reference: the
 * DataLoader + collate_fn_train / collate_fn_pretrain of src/data/dataset.py:139-161 with the `.to(device)` of
 * train.py:117 / pretrain.py:56; the host collates (data.py) are unchanged.
 *
 * Conventions are those of vs_scorer.h: every pointer is a DEVICE pointer unless stated otherwise, the work is enqueued on
 * the caller's stream, nothing allocates, copies to or from the host or synchronises, every function returns 0 or a VS_ERR_*
 * status and sets vs_last_error(), and every argument check runs on the host before any HIP call.
 *
 * A batch is described by two device arrays, so the plan of a whole epoch is uploaded once and every call takes pointers
 * into it:
 *   ids       int32 [B]     the videos of the batch (indices into video_start), in batch order; an id may repeat
 *   out_start int32 [B + 1] out_start[0] = 0, out_start[b + 1] = out_start[b] + length of video ids[b]
 * with the set's  video_start int64 [V + 1]  (video v = arena rows [video_start[v], video_start[v + 1])).  The host
 * integers that bound the output (total_rows = out_start[B]; t_max, longest) are passed beside them: the kernel never
 * writes outside the output those integers describe, whatever the device arrays hold, and it clamps every id to [0, V)
 * and every source row to [0, video_start[V]), so a wrong plan gives wrong rows, never an access outside the arena.  (A
 * video_start whose last entry is not positive describes an empty arena: nothing is read, and the packed form then writes
 * pad rows - 0.0 - like the padded form beyond a video's end.)
 *
 * The kernels are pure copies: 16-byte accesses when the row width is a multiple of 4 floats and every feature pointer is
 * 16-byte aligned, 4-byte accesses otherwise (same results).  The grid is capped (2048 blocks) and strides over the rest;
 * the results do not depend on it.
 */
#ifndef VS_BATCH_H
#define VS_BATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* PACKED batch (the tuple of collate_fn_train_packed): out[out_start[b] + t][:] = arena[video_start[ids[b]] + t][:] and
 * side_out[out_start[b] + t] = side[video_start[ids[b]] + t] for t < out_start[b + 1] - out_start[b], one launch for both.
 *   arena     float [N_total][d]          side_or_null  float [N_total] (with side_out_or_null; both or neither)
 *   out       float [total_rows][d]       side_out      float [total_rows]
 *   n_videos = V >= 1, B >= 1, d >= 1, 1 <= total_rows < 2^31 (HOST integers; total_rows must equal out_start[B]). */
int vs_batch_gather_packed(const float *arena, const float *side_or_null, const int64_t *video_start, int32_t n_videos,
                           const int32_t *ids, const int32_t *out_start, int32_t B, int64_t total_rows, int32_t d,
                           float *out, float *side_out_or_null, void *stream);

/* PADDED batch (collate_fn_train + `mask = feature[:, :, 0] == 1000`): for t < length of video ids[b] the row and its side
 * value as above at out[b][t][:], side_out[b][t], mask 0; for length <= t < t_max all d columns and the side value hold
 * pad_value and the mask is 1.  One launch writes the three outputs.
 *   out  float [B][t_max][d]     side_out_or_null  float [B][t_max]     mask_out_or_null  uint8 [B][t_max]
 *   longest: HOST integer, the longest video of the batch (the caller's plan knows it); t_max >= longest >= 1 is checked
 *   here, and the kernel cuts a longer video at t_max.  out_start as for the packed form (it gives the lengths). */
int vs_batch_gather_padded(const float *arena, const float *side_or_null, const int64_t *video_start, int32_t n_videos,
                           const int32_t *ids, const int32_t *out_start, int32_t B, int32_t longest, int32_t t_max,
                           float pad_value, int32_t d, float *out, float *side_out_or_null, uint8_t *mask_out_or_null,
                           void *stream);

/* Row gather: out[b][:] = table[ids[b]][:] (the 512-wide video representations of a pretraining batch).
 *   table float [n_rows][w]     ids int32 [B]     out float [B][w]     n_rows >= 1, B >= 1, w >= 1. */
int vs_batch_gather_rows(const float *table, int32_t n_rows, const int32_t *ids, int32_t B, int32_t w, float *out,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VS_BATCH_H */
