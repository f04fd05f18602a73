/*
 * vs_inspect.h — C ABI of the attention maps: the softmax weights of the scorer's self-attention layers, on request.
 * Replaces: the `attention_maps` list of the reference's encoder (simnet.py:112-113, the tensor MultiAttentionNetwork.forward
 * returns beside its output, :155-164) and what train.py:155-165 would dump from it.
 *
 * The scoring entry points (vs_scorer.h) never form the [N,N] weights; these do, for the layers asked for, as an exact
 * fp32 side computation on the q / k planes the forward already leaves in its workspace (csrc/vs_attention_maps.hip).  For
 * layer l, video b, head h, with N = T (T + 1 with a class token: the token is position 0 and never padding):
 *     P[i, j]     = softmax_j(q_i . k_j * d_model^-0.5, key j padding -> -inf)   eval mode, before dropout; a masked key
 *                   column is exactly 0.0f; padded QUERY rows are computed like any other row
 *     received[j] = (1 / n_b) * sum over the n_b non-padding queries i of P[i, j]   (sums to 1 over j)
 *     entropy[i]  = -sum_j P[i, j] log P[i, j], nats, 0 log 0 = 0
 * `received` and `entropy` never store [N,N]: they are the form for long videos.  No atomics: two calls give the same
 * bits, and a video's maps do not depend on the batch it is in.  A video whose keys are all masked is outside the
 * contract, as it is for vs_scorer_forward.
 *
 * All pointers are device pointers unless marked HOST.  Every function returns 0 or a VS_ERR_* status and sets
 * vs_last_error(); the argument checks need no GPU.  Work is enqueued on `stream`; nothing synchronises.
 */
#ifndef VS_INSPECT_H
#define VS_INSPECT_H

#include "vs_scorer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device bytes vs_inspect_forward needs: the forward's own workspace (vs_scorer_workspace_bytes, or _cls when
 * with_cls != 0) plus one float per (video, head, position).  0: invalid arguments. */
size_t vs_inspect_workspace_bytes(const vs_weights *w, int32_t B, int32_t T, int32_t with_cls);

/* vs_scorer_forward (cls_token == NULL) or vs_scorer_forward_cls with flags 0 - the exact fp32 kernels, raw logits -
 * plus a read-only look at the q / k planes of every selected layer: `scores` and `hidden` are bit-identical to those
 * calls on the same input.
 * layers: HOST [n_layers], strictly ascending, each in [0, num_layers).  N = T, or T + 1 when cls_token != NULL.
 * maps [n_layers, B, H, N, N], received [n_layers, B, H, N], entropy [n_layers, B, H, N]: any may be NULL, not all three.
 * x, hidden, cls_token and the three outputs 16-byte aligned, workspace 256-byte aligned. */
int vs_inspect_forward(const vs_weights *w, const float *x, const uint8_t *key_pad_mask, const float *cls_token,
                       int32_t B, int32_t T, const int32_t *layers, int32_t n_layers,
                       float *scores, float *hidden, float *maps, float *received, float *entropy,
                       void *workspace, size_t workspace_bytes, void *stream);

/* The kernels alone, for parity tests: q, k head-major [B, H, T, dh] fp32 (the planes vs_qkv_proj_f32 writes), dh 32 /
 * 64 / 128 / 256, key_pad_mask [B, T] or NULL (it also tells which QUERIES count in `received`), scale as in
 * vs_attention_f32.  maps [B, H, T, T], received [B, H, T], entropy [B, H, T]: any may be NULL, not all three. */
size_t vs_attention_probs_workspace_bytes(int32_t B, int32_t H, int32_t T);
int vs_attention_probs_f32(const float *q, const float *k, const uint8_t *key_pad_mask, float *maps, float *received,
                           float *entropy, int32_t B, int32_t H, int32_t T, int32_t dh, float scale, void *workspace,
                           size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VS_INSPECT_H */
