/*
 * vs_inspect_packed.h - C ABI of the attention maps (vs_inspect.h) on PACKED ragged batches: the softmax weights of the
 * scorer's self-attention layers and their two streamed reductions for a set of videos of different lengths, with no padded
 * row and no mask.  Replaces: the loop of the reference's save_attention_weights over a whole loader (train.py:155-165).
 *
 * The mathematics, the two-pass kernels and the general rules are those of vs_inspect.h: device pointers unless marked HOST,
 * every function returns 0 or a VS_ERR_* status and sets vs_last_error(), the argument checks need no GPU, work is enqueued
 * on `stream`, nothing synchronises.  This header lives in include/packed/ and is bound by its own table
 * (_lib._PACKED_INSPECT_BINDINGS): an addition beside the ABI of include/*.h, which it leaves exactly as it was.
 */
#ifndef VS_INSPECT_PACKED_H
#define VS_INSPECT_PACKED_H

#include "../vs_inspect.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- packed ragged batches: the videos' frames concatenated, no padded row, no mask (vs_scorer_forward_packed) ----
 * lengths: HOST [B], each > 0 (and within the positional table); lengths_dev: the same values on the device.  M = sum of
 * the lengths, video b = packed rows cu[b] .. cu[b+1]-1 with cu the running sum.  Head dim 32 / 64 / 128 and no class token,
 * as for vs_scorer_forward_packed (anything else: VS_ERR_INVALID).  Layouts:
 *     received, entropy  [H, M] per layer, packed like the frames; every query of a packed video is valid, so `received`
 *                        divides by n_b = T_b
 *     maps               per layer the videos' [H, T_b, T_b] blocks one after the other, video-major: video b starts at
 *                        float offset H * sum over u < b of T_u^2 - a 64-bit quantity (it passes 2^31 for long videos);
 *                        H * sum T_b^2 floats per layer instead of the padded form's B * H * Tmax^2
 * A wave's unit of work is (head, video, 32-row tile of THAT video): the tile walk starts at the video's own first row, rows
 * past its end re-read its own last row (no load passes row M - 1 of a plane).  No atomics: two calls give the same bits, a
 * video's result does not depend on what it is packed with, and it is bit for bit what vs_attention_probs_f32 gives for that
 * video alone (B = 1, T = T_b, no mask).  The (video, tile) list, cu and the map offsets are built on the device from
 * lengths_dev; the host lengths only size the launch: no host memory is read after the call returns, nothing synchronises. */

/* Device bytes vs_inspect_forward_packed needs: vs_scorer_workspace_bytes_packed plus one float per (head, packed row) plus
 * the plan of sum ceil(T_b / 32) (video, tile) pairs.  0: invalid arguments. */
size_t vs_inspect_workspace_bytes_packed(const vs_weights *w, const int32_t *lengths, int32_t B);

/* vs_scorer_forward_packed with flags 0 - `scores` [M, num_classes] and `hidden` [M, d_model] (or NULL) are bit-identical to
 * that call - plus the packed map kernels on the q / k planes of every selected layer.
 * layers: HOST [n_layers], strictly ascending, each in [0, num_layers).
 * maps [n_layers] x (H * sum T_b^2), received [n_layers, H, M], entropy [n_layers, H, M]: any may be NULL, not all three.
 * x, hidden and the three outputs 16-byte aligned, workspace 256-byte aligned. */
int vs_inspect_forward_packed(const vs_weights *w, const float *x, const int32_t *lengths, const int32_t *lengths_dev, int32_t B,
                              const int32_t *layers, int32_t n_layers, float *scores, float *hidden, float *maps, float *received,
                              float *entropy, void *workspace, size_t workspace_bytes, void *stream);

/* The packed kernels alone, for parity tests: q, k head-major [H, M, dh] fp32, dh 32 / 64 / 128, scale as in vs_attention_f32.
 * maps (H * sum T_b^2 floats), received [H, M], entropy [H, M]: any may be NULL, not all three. */
size_t vs_attention_probs_packed_workspace_bytes(const int32_t *lengths, int32_t B, int32_t H);
int vs_attention_probs_packed_f32(const float *q, const float *k, const int32_t *lengths, const int32_t *lengths_dev, int32_t B,
                                  int32_t H, int32_t dh, float scale, float *maps, float *received, float *entropy,
                                  void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VS_INSPECT_PACKED_H */
