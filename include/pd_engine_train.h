/*
 * pd_engine_train.h -- the training branch with gradients: GaussianDiffusion.p_losses (models/gaussian_diffuser.py:308-327) forward
 * AND backward through the Denoiser (models/denoiser.py:53-76) on hand-written gfx950 kernels (csrc/pd_train.hip).
 *
 * An extension header like pd_engine_ingest.h: the function list of pd_engine.h is pinned.  The surface is a separate opaque object,
 * pd_trainer; pd_engine and all its launches are untouched.
 *
 * What a trainer is
 *   - it keeps NO weight copy: every call reads the caller's LIVE tensors (DEVICE pointers, PyTorch layout [out, in]) through the
 *     pd_weights it is handed, so an optimiser step needs no rebuild and no repacking;
 *   - it owns one activation stash sized at creation for max_B x max_N token rows, and the two q_sample tables;
 *   - exact fp32 everywhere (v_mfma_f32_32x32x2_f32), pre-norm only, N <= 64 frames by default, up to 256 with PD_TR_OPT_MAX_FRAMES,
 *     head dim <= 128, pivot column on or off, both objectives, both loss types; pd_train_forward is the eval-mode function, pd_train_forward_dropout the .train()-mode one with the
 *     encoder layers' dropout (masks from a counter-based generator, recomputed by the backward, never stored);
 *   - no float atomics in any reduction: gradients are bitwise reproducible and do not depend on the trainer's capacity (every
 *     reduction over token rows is chunked by a function of M = B x N alone and its partial sums are added in chunk order);
 *   - three outputs of the forward are differentiable: loss, model_out and x_0_pred (pd_train_backward_ex takes an upstream gradient of
 *     each; pd_train_backward is the loss alone); x_t is data.  pd_pose_to_camera_backward takes a loss on the cameras decoded from
 *     x_0_pred back to x_0_pred;
 *   - the image backbone is not this object's: dz is handed back for whoever owns z -- pd_vit_trainer (pd_engine_vit_train.h) takes it on
 *     to the backbone's parameters.
 * Conventions are those of pd_engine.h (return codes, pd_last_error, `stream` = hipStream_t as void *).  Both calls are asynchronous on
 * `stream`; after pd_trainer_create nothing synchronises with the host and nothing is allocated.
 */
#ifndef PD_ENGINE_TRAIN_H
#define PD_ENGINE_TRAIN_H

#include "pd_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pd_trainer pd_trainer;

/* mirrors pd_layer_weights: where the gradient of each tensor goes (DEVICE fp32, the parameter's own layout); NULL = not wanted */
typedef struct pd_layer_grads {
    float *norm1_w, *norm1_b;
    float *in_proj_w, *in_proj_b;
    float *out_proj_w, *out_proj_b;
    float *norm2_w, *norm2_b;
    float *linear1_w, *linear1_b;
    float *linear2_w, *linear2_b;
} pd_layer_grads;

/* mirrors the weight members of pd_weights */
typedef struct pd_weight_grads {
    float *time_w0, *time_b0, *time_w2, *time_b2, *first_w, *first_b;
    pd_layer_grads layers[PD_MAX_LAYERS];
    float *last0_w, *last0_b, *last_ln_w, *last_ln_b, *last3_w, *last3_b;
} pd_weight_grads;

/* Reads only the shape fields, the flags and the schedule tables of `shape` (no weight pointer is touched) and copies the two q_sample
 * tables ([timesteps] DEVICE fp32 each, gaussian_diffuser.py:164-165) plus shape->sqrt_recip / sqrt_recipm1_alphas_cumprod (x_0_pred
 * under pred_noise; NULL there makes x0_pred_out unavailable).  Sizes the stash for max_B x max_N token rows.  Synchronous.
 * PD_ERR_UNSUPPORTED, naming the limit, for PD_WEIGHTS_POST_NORM, a head dim above 128, and anything outside pd_weights' family. */
int pd_trainer_create(const pd_weights *shape, const float *sqrt_alphas_cumprod, const float *sqrt_one_minus_alphas_cumprod,
                      int max_B, int max_N, pd_trainer **out);
void pd_trainer_destroy(pd_trainer *tr);

/* Per-trainer options.  N <= 64 runs the attention kernels that hold a (sequence, head) whole in LDS; N > 64 runs the key-tiled kernels
 * (K and V through LDS in tiles of 64 keys; the backward in two launches with 16 nhead bytes of row statistics per token row, sized at
 * pd_trainer_create).  At N <= 64 the key-tiled kernels perform the same operations on the same operands in the same order and give the
 * same bits; PD_TR_OPT_LONG_ATTN = 1 runs them there.  The trainer remembers with the pending stash which family its forward ran, and the
 * backward uses that family even if an option changed in between.  Synchronous, allocates nothing.  Any other option or value:
 * PD_ERR_INVALID_ARG naming it, the old value stays in force. */
#define PD_TR_OPT_MAX_FRAMES 1   /* 64 (default) .. 256 (PD_MAX_DENOISER_FRAMES): frames per sequence pd_train_forward admits        */
#define PD_TR_OPT_LONG_ATTN  2   /* 0 (default): N <= 64 runs the short kernels, N > 64 the key-tiled ones; 1: key-tiled at every N */
int pd_trainer_set_option(pd_trainer *tr, int option, int value);
int pd_trainer_get_option(pd_trainer *tr, int option, int *value);

/* Sequences of different frame counts in one padded batch -- the trainer's pd_engine_set_frame_counts.  n_frames: HOST int32 [B], each in
 * [1, N of the later forward]; NULL or B == 0 clears.  Ordered on `stream`: the counts travel as kernel arguments of a small launch into
 * a device array sized for max_B at pd_trainer_create, so the call neither synchronises nor allocates and the caller's array is free on
 * return; a host copy serves validation.  The frame limit (64, or PD_TR_OPT_MAX_FRAMES) applies to N.  PD_ERR_INVALID_ARG naming the rule:
 * here for B outside [0, max_B] or a count outside [1, min(max_N, 256)]; at a forward whose B differs from the counts' B or whose N is
 * below a count ("every count must lie in [1, N]"), before anything is launched.
 * While counts are set, pd_train_forward, pd_train_forward_dropout and the pd_train_backward of such a forward mean:
 *   layout      sequence b has n_frames[b] frames in rows 0 .. n_frames[b]-1 of its N-row block; the other rows are padding.  Nothing is
 *               packed: the row stride stays N, the pivot column stays at row 0 of each block, and the dropout masks keep their
 *               definition on the PADDED layout (rows (b nhead + h) N + i and m = b N + i with the padded N).
 *   attention   a sequence sees its keys < n_frames[b] only, in the forward and in the backward's recomputation of P.  The key-tiled
 *               kernels serve every N (the short ones hold a uniform batch); at N <= 64 they give the short kernels' bits.
 *   outputs     padding rows of loss, x_0_pred, x_t, model_out and dz_out are +0.0f.
 *   inputs      padding rows of x_start, z, noise and g_loss are never read: valid rows of every output and every parameter gradient
 *               do not depend on what they hold, NaN included.  Every gradient row of a padding row is exactly zero, so it adds nothing
 *               to the weight, bias and LayerNorm sums or to the time embedding's sum over frames.
 *   definition  S = sum of g_loss loss over the valid rows.  Slot b's outputs and dz are, bit for bit, those of sequence b run alone
 *               with N = n_frames[b] (every forward and data-gradient stage is per token row, and attention performs the same operations
 *               on the same operands in the same order); a parameter gradient is the sum over the sequences run alone, up to the order
 *               of its sum over rows (chunked by M = B x N, padding rows included as exact zeros).
 *   pending     the counts of a forward belong to its stash, like the options: the backward uses them even if this function was called
 *               or cleared in between.
 * With no counts set every call launches exactly what it launched before and gives the same bits.  NULL trainer: PD_ERR_INVALID_ARG. */
int pd_trainer_set_frame_counts(pd_trainer *tr, int B, const int32_t *n_frames, void *stream);

/* The contract of pd_p_losses (same outputs, same t_seq clamping -- a clamped timestep raises the trainer's own error word,
 * pd_trainer_check_async) with the weights taken from `w` at the time of the call, and the stash the backward needs:
 * per layer the residual stream at both sublayer inputs, both LayerNorm (mean, rstd) pairs, qkv, ctx and the post-ReLU FF activations;
 * _first's input rows; _last's LayerNorm input, statistics and post-ReLU hidden; the time embedding's SiLU input.  Attention
 * probabilities are recomputed by the backward.  N above the trainer's frame limit (64 by default, PD_TR_OPT_MAX_FRAMES):
 * PD_ERR_UNSUPPORTED, "limit of <v> frames", before anything is launched.  loss_type 1 = l1, 2 = l2. */
int pd_train_forward(pd_trainer *tr, const pd_weights *w, const float *x_start, const float *z, const int64_t *t_seq,
                     const float *noise, int B, int N, int loss_type,
                     float *loss_out, float *x0_pred_out, float *xt_out, float *model_out, void *stream);

/* pd_train_forward with dropout of probability p at the sites in `sites` of every encoder layer -- nn.TransformerEncoderLayer's four:
 *   PD_DROP_ATTN    the attention probabilities, after the softmax and before P V; row (b nhead + h) N + i, column = key j
 *   PD_DROP_RESID1  dropout1, on out_proj(ctx) + bias before the residual add;       row = token row m, column < d_model
 *   PD_DROP_FF      the feed-forward dropout, after linear1's ReLU;                   row m, column < dim_ff
 *   PD_DROP_RESID2  dropout2, on linear2(..) + bias before the residual add;          row m, column < d_model
 * (_last and the time embedding have none in the reference).  The element at (row r, column c) of site s (0 .. 3 in the order above) of
 * layer l is KEPT iff word r & 3 of philox4x32_10(counter = (r >> 2, c, 4 l + s, step), key = (seed & 0xffffffff, seed >> 32)) is
 * >= floor(p 2^32); kept values are multiplied by the fp32 value 1 / (1 - p).  The mapping depends on (B, N) and the network shape
 * alone, never on the trainer's capacity.  The trainer remembers (p, sites, seed, step) with the pending stash: pd_train_backward
 * differentiates THIS function, recomputing every mask.  The stashed FF activations are post-dropout (what linear2 read).
 * p == 0 or sites == 0 is pd_train_forward itself: same launches, same bits.  p outside [0, 1) or NaN, or a bit of `sites` outside
 * PD_DROP_ALL: PD_ERR_INVALID_ARG naming the argument, before anything is launched. */
#define PD_DROP_ATTN 1u
#define PD_DROP_RESID1 2u
#define PD_DROP_FF 4u
#define PD_DROP_RESID2 8u
#define PD_DROP_ALL 15u
int pd_train_forward_dropout(pd_trainer *tr, const pd_weights *w, const float *x_start, const float *z, const int64_t *t_seq,
                             const float *noise, int B, int N, int loss_type, float p, unsigned sites, uint64_t seed, uint32_t step,
                             float *loss_out, float *x0_pred_out, float *xt_out, float *model_out, void *stream);

/* With S = sum(g_loss * loss) over the [B, N, 9] elements: writes dS/dtheta for every non-NULL member of `grads` (an overwrite, in the
 * parameter's own layout; a NULL member's weight-gradient launch is not issued) and dS/dz [B, N, z_dim] when dz_out is non-NULL.
 * Loss derivative: sign(d) with sign(0) = 0 (l1), 2 d (l2), d = model_out - target; x_0_pred and model_out carry no gradient here
 * (pd_train_backward_ex takes theirs).
 * After pd_train_forward_dropout it differentiates that call's function (same masks).
 * Consumes the stash: PD_ERR_STATE when no forward is pending.  `w` must point to the same unmodified tensors as the forward's.
 * It is pd_train_backward_ex(tr, w, g_loss, NULL, NULL, grads, dz_out, stream): the same launches, the same bits. */
int pd_train_backward(pd_trainer *tr, const pd_weights *w, const float *g_loss, const pd_weight_grads *grads, float *dz_out,
                      void *stream);

/* pd_train_backward with upstream gradients of the other two differentiable outputs of the forward:
 *   S = sum(g_loss * loss) + sum(g_model_out * model_out) + sum(g_x0_pred * x_0_pred)   over the valid rows,
 * each upstream [B, N, 9] DEVICE fp32, each may be NULL (the term is absent); all three NULL: PD_ERR_INVALID_ARG.  x_t is data.
 * The row vector that enters _last.3 is the sum of the PRESENT terms in this order -- an absent term is not added, not even as "+ 0":
 *   g_loss * dl,   g_model_out,   k_b * g_x0_pred
 * with k_b = 1 under pred_x0 (x_0_pred is model_out) and k_b = -sqrt_recipm1_alphas_cumprod[t_b] under pred_noise (x_0_pred =
 * sqrt_recip x_t - sqrt_recipm1 model_out; the fp32 table copied at pd_trainer_create, at the forward's clamped t).  One term alone is
 * that single fp32 product, or the plain value for g_model_out (and for g_x0_pred under pred_x0).  g_x0_pred under pred_noise on a
 * trainer created without the recip tables: PD_ERR_STATE naming them, before anything is launched (the stash stays pending).
 * Padding rows of all three upstreams are never read, NaN included; the row vector is zero there.
 * Everything else is pd_train_backward's contract: it consumes the stash, uses the forward's pending attention family, frame counts and
 * dropout masks, skips the launches of NULL members of `grads`, and uses no float atomics. */
int pd_train_backward_ex(pd_trainer *tr, const pd_weights *w, const float *g_loss, const float *g_model_out, const float *g_x0_pred,
                         const pd_weight_grads *grads, float *dz_out, void *stream);

/* Backward of pd_pose_to_camera_ex (pose_encoding_to_camera, util/camera_transform.py:64-105).  Stateless like pd_camera_to_pose: no
 * pd_engine.  The decode is recomputed from enc [n, 9] with the forward kernel's expressions; g_R [n, 9], g_T [n, 3], g_focal [n, 2]
 * (DEVICE fp32) may each be NULL (= zero), not all three.  g_enc_out [n, 9]:
 *   columns 0-2  g_T, copied;
 *   columns 3-6  the gradient through pytorch3d's quaternion_to_matrix (real part first, two_s = 2 / |q|^2, no normalisation);
 *   columns 7-8  g_focal * f where min <= f = exp(logFL + bias) <= max, 0 outside (torch.clamp passes the gradient on the closed
 *                interval).
 * One thread per camera, the forward's grid.  PD_ERR_INVALID_ARG naming the function for NULL enc / g_enc_out, n_cameras <= 0 or
 * all-NULL upstreams. */
int pd_pose_to_camera_backward(const float *enc, const float *g_R, const float *g_T, const float *g_focal,
                               int n_cameras, float log_focal_length_bias, float min_focal_length,
                               float max_focal_length, float *g_enc_out, void *stream);

/* The tests' window into the stash of the pending (or last) forward: layer < num_layers -> that layer's [B x N, dim_ff] post-ReLU FF
 * activations; layer == num_layers -> _last's [B x N, mlp_hidden] post-ReLU values.  n_floats must be exactly that size.  The stash is
 * returned as it is: after pd_train_forward_dropout with PD_DROP_FF an encoder layer's values are POST-dropout (0 where dropped, times
 * 1 / (1 - p) where kept). */
int pd_train_debug_relu(pd_trainer *tr, int layer, float *dst, long long n_floats, void *stream);

/* Synchronises the device; PD_ERR_STATE if pd_train_forward met (and clamped) a timestep outside [0, timesteps) since the last check. */
int pd_trainer_check_async(pd_trainer *tr);

#ifdef __cplusplus
}
#endif
#endif /* PD_ENGINE_TRAIN_H */
