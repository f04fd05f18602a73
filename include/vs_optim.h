/*
 * vs_optim.h — C ABI of the parameter update of libvsscore.so: the last line of the reference's training step
 *     scaler.step(optim)        reference src/train.py:128 with optim = torch.optim.Adam(...) (train.py:35, pretrain.py:35)
 * as ONE multi-tensor HIP launch per group of up to VS_ADAM_MAX_TENSORS tensors.  The arithmetic is torch.optim.Adam's
 * in fp32:
 *     g' = g / grad_scale (when a scale is given) + weight_decay * p        (L2 decay; see `decoupled`)
 *     m  = m + (1 - beta1) (g' - m)            v = beta2 v + (1 - beta2) g'^2
 *     p  = p - (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * with t the number of steps taken INCLUDING this one.  t lives on the device (one fp32 count per tensor, as torch's
 * fused / capturable form keeps it) and advances only on a step that was not skipped.
 *
 * Loss scaling (torch.amp.GradScaler, train.py:60,126-128): `grad_scale` and `found_inf` are DEVICE fp32 scalars, either
 * may be NULL.  With *found_inf != 0 the launch leaves p, m, v, the packed copy and the step counts bit-for-bit unchanged.
 * The host never reads either: no call here synchronises, allocates or copies to the host.
 *
 * Same conventions as vs_scorer.h: device pointers, work enqueued on the caller's stream, int status + vs_last_error().
 * Tensors may have any length and alignment (16-byte vector accesses where all pointers of a tensor allow them, an
 * element-wise path otherwise).  Results do not depend on how the tensors are grouped into launches: a step is bitwise
 * reproducible.
 */
#ifndef VS_OPTIM_H
#define VS_OPTIM_H

#include "vs_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Hyper-parameters, passed with their CURRENT values on every call: a scheduler that rewrites lr per step (reference
 * src/schedular.py:20-25) needs nothing else.  Doubles, as torch holds them (Python floats): (float)(1 - beta1) and
 * 1 - (float)beta1 differ by 2e-7 relative, which is more than the update's own rounding. */
typedef struct vs_adam_cfg {
    double lr;
    double beta1, beta2;     /* in [0, 1) */
    double eps;
    double weight_decay;     /* >= 0 */
    int32_t decoupled;       /* 0: torch.optim.Adam (L2: added to the gradient); 1: AdamW (p *= 1 - lr * weight_decay) */
    int32_t reserved;        /* 0 */
} vs_adam_cfg;

/* One tensor of the generic entry.  `mirror` (or NULL) is a second destination of the new p; `step` points to the
 * tensor's fp32 step count (t - 1 before the call).  No two entries of a call may share p, m, v or step. */
typedef struct vs_adam_tensor {
    float *p;
    const float *g;
    float *m, *v;
    float *mirror;
    float *step;
    size_t n;                /* elements (< 2^32) */
} vs_adam_tensor;

#define VS_ADAM_MAX_TENSORS 64      /* per launch; a call with more tensors issues ceil(n / 64) launches */

/* Adam on tensors that belong to no vs_weights handle.  `table`: HOST array of n_tensors entries (read before the call
 * returns).  `sync_word`: one device uint32, zero before the first call and left zero by every launch (the block that
 * finishes last advances the step counts; the word counts the finished blocks).  One sync_word serves any number of calls
 * on one stream. */
int vs_adam_step_tensors(const vs_adam_tensor *table, int32_t n_tensors, const vs_adam_cfg *cfg, const float *grad_scale,
                         const float *found_inf, void *sync_word, void *stream);

/* Adam state of every parameter of a handle: m, v (zero) and the step counts (zero) in ONE caller-owned device buffer of
 * vs_adam_state_bytes(w) bytes, 256-byte aligned.  vs_adam_state_init zeroes it, stream-ordered. */
size_t vs_adam_state_bytes(const vs_weights *w);
int vs_adam_state_init(const vs_weights *w, void *state, void *stream);

/* Where a tensor's state lives inside that buffer (a binding that wants views of it, e.g. for a checkpoint): tensor
 * index in vs_model_params order - 0 embed_w, 1 embed_b, 2 + 16 l + j the j-th field of vs_layer_params of layer l,
 * 2 + 16 L final_w, 3 + 16 L final_b; which 0 = m, 1 = v, 2 = step count.  Byte offset and element count. */
int vs_adam_state_field(const vs_weights *w, int32_t tensor, int32_t which, size_t *offset_bytes, size_t *count);

/* One Adam step on the parameters of a handle.  `grads`: what vs_train_backward filled; a NULL gradient pointer leaves
 * that tensor (parameter, state, step count) untouched, so a subset can be optimised.
 *   params == NULL: the packed copy inside the handle is the only copy of the parameters (a plain-C client) and is
 *                   updated in place;
 *   params given:   the caller's tensors (e.g. the torch parameters, which must hold the values the handle was packed
 *                   from) are updated AND the new values are stored into the packed copy by the same launch, so no
 *                   vs_weights_update is needed afterwards.  params->pos_embedding is ignored (a buffer).
 * Either way the handle counts as updated exactly as after vs_weights_update: the kernel-layout images and the training
 * path's transposes are rebuilt lazily by their next reader, and calls on other streams are ordered behind this one.
 * Not for a handle that embeds a narrower model (vs_weights_set_norm_width): its tensors are not the caller's. */
int vs_adam_step(vs_weights *w, const vs_model_params *params, const vs_model_grads *grads, void *state,
                 const vs_adam_cfg *cfg, const float *grad_scale, const float *found_inf, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VS_OPTIM_H */
