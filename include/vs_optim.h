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

/* ---- Clipping the global gradient norm (torch.nn.utils.clip_grad_norm_) without rewriting the gradients ----------------
 * The Adam kernel divides every gradient by the device scalar `grad_scale`.  The calls below measure the norm of ALL
 * gradients of a step and write, next to it, the divisor grad_scale / clip_coef: handing THAT scalar to vs_adam_step* as
 * its grad_scale is the clipped step - one extra read of the gradients, no write.
 *     out[0]  total norm of the unscaled gradients: sqrt(sum g^2) / grad_scale, or max |g| / grad_scale
 *     out[1]  clip_coef = min(1, max_norm / (out[0] + 1e-6)) (torch's formula); exactly 1 when nothing is clipped
 *     out[2]  grad_scale / clip_coef (1 / clip_coef without a scale); bit-equal to grad_scale whenever out[1] == 1
 *     out[3]  0
 * Squares are summed in double in a fixed order: the result is bitwise reproducible and does not depend on the grouping
 * of the tensors into launches or on their alignment.  IEEE rules throughout (torch with error_if_nonfinite=False): an
 * infinite norm gives clip_coef 0, a NaN norm NaN.  `grad_scale`: device scalar or NULL.  max_norm = +inf measures only.
 * Launches: ceil(tensors / 64) + 1.  VS_ERR_INVALID (before any device access): NULL table / out / workspace, max_norm
 * NaN or <= 0, unknown kind, n >= 2^32, workspace not 8-byte aligned.  VS_ERR_WORKSPACE: workspace too small. */
typedef struct vs_grad_tensor { float *g; size_t n; } vs_grad_tensor;   /* g NULL or n 0: skipped; n < 2^32 */
#define VS_GRAD_NORM_L2  0
#define VS_GRAD_NORM_MAX 1

/* host only; a non-zero multiple of 256, or 0 on invalid input (NULL table, n_tensors < 0, n >= 2^32) */
size_t vs_grad_norm_workspace_bytes(const vs_grad_tensor *table, int32_t n_tensors);

/* `table`: HOST array (read before the call returns); `out`: 4 device floats; `workspace`: device, caller-owned */
int vs_grad_norm_tensors(const vs_grad_tensor *table, int32_t n_tensors, int32_t kind, double max_norm,
                         const float *grad_scale, float *out, void *workspace, size_t workspace_bytes, void *stream);

/* The gradients of a handle: tensors in vs_model_params order with the handle's sizes, NULL gradient pointers skipped.
 * The workspace is that of a vs_grad_tensor table with the same sizes.  Not for a handle that embeds a narrower model. */
int vs_grad_norm(const vs_weights *w, const vs_model_grads *grads, int32_t kind, double max_norm,
                 const float *grad_scale, float *out, void *workspace, size_t workspace_bytes, void *stream);

/* g *= *coef in place (`coef`: device scalar, e.g. out + 1); nothing is written when *coef == 1.  For a loop that keeps
 * another optimizer: vs_grad_norm_tensors, then this. */
int vs_grad_scale_tensors(const vs_grad_tensor *table, int32_t n_tensors, const float *coef, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VS_OPTIM_H */
