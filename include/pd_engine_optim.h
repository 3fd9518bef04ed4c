/*
 * pd_engine_optim.h -- the optimiser step of training (the reference's train.py:247-250: clip_grad_norm_ over model.parameters(), then
 * torch.optim.AdamW.step()) on hand-written gfx950 kernels (csrc/pd_optim.hip): the global L2 norm of the gradients,
 * the clip coefficient and the decoupled-weight-decay Adam update, in two passes over the tensors.
 *
 * An extension header like pd_engine_train.h: the function list of pd_engine.h is pinned.  The surface is one more opaque object,
 * pd_optimizer; no other object and none of their launches is touched.
 *
 * What an optimizer object is -- the rules of the trainers:
 *   - it keeps NO copy of any tensor: every call works on the caller's LIVE device tensors, named by a HOST array of pd_optim_tensor that is
 *     read during the call and sent to the device by value in kernel arguments, ordered on `stream` (two calls issued back to back cannot
 *     overwrite each other's table, and a call may name other tensors than the one before: fresh gradient tensors every step are the rule);
 *   - capacity is fixed at creation (tensors per call, elements per call); after pd_optimizer_create nothing allocates and nothing
 *     synchronises with the host; the clip coefficient never leaves the device;
 *   - no float atomics: the squared norm is accumulated in fp64, one partial sum per chunk of PD_OPTIM_CHUNK elements of one tensor, and
 *     the partial sums are added in an order fixed by their number alone.  The norm is bitwise reproducible and depends on the tensors'
 *     sizes and values in call order only -- not on pointer alignment, the launch grid or the object's capacity;
 *   - every element goes through the same fp32 arithmetic whichever way it is loaded (16-byte accesses when a tensor's pointers are all
 *     16-byte aligned, 4-byte ones otherwise).
 * One object serves one stream at a time (its partial sums and coefficient are its own); calls on it are ordered on `stream`.
 * Conventions are those of pd_engine.h (return codes, pd_last_error, `stream` = hipStream_t as void *).
 */
#ifndef PD_ENGINE_OPTIM_H
#define PD_ENGINE_OPTIM_H

#include "pd_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pd_optimizer pd_optimizer;

#define PD_OPTIM_CHUNK 4096   /* elements of one tensor per partial sum and per workgroup turn; a multiple of 4, so a chunk keeps its tensor's alignment */

/* one parameter that has a gradient this step: DEVICE fp32, contiguous, numel values each.  pd_optim_grad_norm and
 * pd_optim_clip_grad_norm read `grad` and `numel` only. */
typedef struct pd_optim_tensor {
    float *param, *grad, *exp_avg, *exp_avg_sq;
    int64_t numel;
    int32_t group;   /* index into the call's pd_optim_group array */
    int32_t step;    /* this tensor's step count AFTER this step (>= 1): the bias corrections are 1 - beta^step */
} pd_optim_tensor;

typedef struct pd_optim_group {
    double lr, beta1, beta2, eps, weight_decay;
} pd_optim_group;

/* Capacity: max_tensors entries per call, max_numel_total elements summed over the tensors of one call.  Synchronous. */
int pd_optimizer_create(int max_tensors, int64_t max_numel_total, pd_optimizer **out);
void pd_optimizer_destroy(pd_optimizer *o);

/* norm_out[0] (DEVICE fp32) = sqrt(sum over the n tensors, in call order, of sum_i grad_i^2): squares and sum in fp64, the square root in
 * fp64, one rounding to fp32.  inf and NaN propagate.  n = 0 gives 0.
 * Every call: PD_ERR_UNSUPPORTED naming the limit, before anything is launched, for n above max_tensors or more elements than
 * max_numel_total; PD_ERR_INVALID_ARG naming the argument for a NULL pointer, numel < 0 and (pd_optim_adamw_step) a group index out of
 * range, step < 1, a beta outside [0, 1), a negative or non-finite lr, eps or weight_decay. */
int pd_optim_grad_norm(pd_optimizer *o, const pd_optim_tensor *t, int n, float *norm_out, void *stream);

/* torch.nn.utils.clip_grad_norm_ for the L2 norm (error_if_nonfinite=False): the norm as above, coef = clamp(max_norm / (norm + 1e-6),
 * max = 1) in fp32 with torch.clamp's NaN rule (a NaN norm gives a NaN coefficient, an inf norm 0), then grad <- grad * coef IN PLACE.
 * norm_out (DEVICE, may be NULL) receives the norm before clipping. */
int pd_optim_clip_grad_norm(pd_optimizer *o, const pd_optim_tensor *t, int n, double max_norm, float *norm_out, void *stream);

/* One step of torch.optim.AdamW (amsgrad=False, maximize=False) on the n tensors, after clipping by the global norm when max_norm > 0
 * (max_norm <= 0: no clipping and no norm pass unless norm_out is given).  Per element, in fp32, with g' = g * coef (g without clipping):
 *     p <- p * (1 - lr wd);  m <- beta1 m + (1 - beta1) g';  v <- beta2 v + (1 - beta2) g'^2;
 *     p <- p - (lr / (1 - beta1^step)) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * The scalars of a (group, step) pair are formed in double and handed to the kernel as fp32.  `grad` is left unchanged.
 * g: HOST array [n_groups].  norm_out (DEVICE, may be NULL) receives the norm before clipping. */
int pd_optim_adamw_step(pd_optimizer *o, const pd_optim_tensor *t, int n, const pd_optim_group *g, int n_groups, double max_norm,
                        float *norm_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PD_ENGINE_OPTIM_H */
