/*
 * pd_engine_vit_train.h -- the image backbone with gradients: MultiScaleImageFeatureExtractor (models/image_feature_extractor.py:57-87)
 * around the DINO ViT-S/16, forward AND backward, on hand-written gfx950 kernels (csrc/pd_vit_train.hip).
 *
 * An extension header like pd_engine_train.h: the function list of pd_engine.h is pinned.  The surface is a second opaque trainer object,
 * pd_vit_trainer; pd_vit, pd_trainer and all their launches are untouched.  It computes z = the averaged CLS features of the images and,
 * given g_z = dS/dz (what pd_train_backward hands back as dz_out), dS/dtheta for every backbone parameter.  Images are data: no image
 * gradient is computed.
 *
 * What a ViT trainer is -- the rules of pd_trainer:
 *   - it keeps NO weight copy: every call reads the caller's LIVE tensors (DEVICE pointers in DINO's state-dict layout) through the
 *     pd_vit_weights it is handed, so an optimiser step needs no rebuild, no LayerNorm folding and no repacking;
 *   - it owns one activation stash, sized at creation for a number of images and of token rows SUMMED over the scales of one call;
 *   - exact fp32 everywhere (v_mfma_f32_32x32x2_f32), the key-tiled attention of the denoiser trainer with the image in the place of the
 *     sequence: at most 256 tokens per image and scale (240 x 272 pixels), head dim 64;
 *   - no float atomics in any reduction: gradients are bitwise reproducible and do not depend on the trainer's capacity (every reduction
 *     over token rows is chunked by a function of the scale's row count alone, its partial sums are added in chunk order, and the scales
 *     are added in a fixed order).
 * Conventions are those of pd_engine.h (return codes, pd_last_error, `stream` = hipStream_t as void *).  Both calls are asynchronous on
 * `stream`; after pd_vit_trainer_create nothing synchronises with the host and nothing is allocated.
 */
#ifndef PD_ENGINE_VIT_TRAIN_H
#define PD_ENGINE_VIT_TRAIN_H

#include "pd_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pd_vit_trainer pd_vit_trainer;

#define PD_VIT_TRAIN_MAX_TOKENS 256   /* tokens per image at one scale, CLS included */
#define PD_VIT_TRAIN_MAX_SCALES 8

/* mirrors pd_vit_layer_weights: where the gradient of each tensor goes (DEVICE fp32, the parameter's own layout); NULL = not wanted */
typedef struct pd_vit_layer_grads {
    float *norm1_w, *norm1_b, *qkv_w, *qkv_b, *proj_w, *proj_b, *norm2_w, *norm2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} pd_vit_layer_grads;

/* mirrors the pointer members of pd_vit_weights */
typedef struct pd_vit_weight_grads {
    float *patch_w, *patch_b, *cls_token, *pos_embed, *norm_w, *norm_b;
    pd_vit_layer_grads layers[16];
} pd_vit_weight_grads;

/* Reads only the shape fields of `shape` (no weight pointer is touched).  Capacity: max_images images per call, max_rows token rows summed
 * over the scales of one call (an image of T tokens at a scale is T rows), max_scales scales per call (<= PD_VIT_TRAIN_MAX_SCALES).
 * Synchronous.  PD_ERR_UNSUPPORTED, naming the limit, for a shape outside pd_vit_weights' family (dim 384, 6 heads, MLP 1536, patch 16,
 * 1 .. 16 blocks, position grid 1 .. 15). */
int pd_vit_trainer_create(const pd_vit_weights *shape, int max_images, int max_rows, int max_scales, pd_vit_trainer **out);
void pd_vit_trainer_destroy(pd_vit_trainer *tr);

/* z_out[n, dim] = mean over the n_scales scales of norm(ViT(rescale(normalise(images))))[:, 0] for images [n, 3, H, W] DEVICE fp32 in
 * [0, 1], with the weights taken from `w` at the time of the call (patch_w [dim, 3, 16, 16] is read as [dim, 768]), and the stash one
 * pd_vit_train_backward consumes: per scale the im2col rows of the prepared images, and per block the residual stream at both sublayer
 * inputs, both LayerNorm (mean, rstd) pairs, qkv, ctx and the fc1 pre-activation; the final LayerNorm's statistics of the CLS rows.
 * Attention probabilities, LayerNorm outputs and GELU outputs are recomputed by the backward.
 * scale_factors: HOST array [n_scales]; a scale of 1 keeps the pixels, another one resizes to floor(H s) x floor(W s) bilinearly
 * (align_corners=False), as pd_vit_forward_scale does.  pos: HOST array [n_scales] of DEVICE pointers: pos[s] = DINO's
 * interpolate_pos_encoding table [1 + gh gw, dim] of scale s's token grid, resampled by the caller from the live pos_embed; NULL = the
 * scale runs on the trained table and reads w->pos_embed itself.  A scale is on the trained table only when its token grid is pos_grid x
 * pos_grid AND its pixel height equals its width (DINO's rule; a table given for such a scale is ignored, it IS pos_embed).  A 224 x 232
 * input has the trained 14 x 14 grid but is resampled by DINO with scale factor 14.1 / 14, which is not a copy: it needs its table, and
 * NULL there is PD_ERR_INVALID_ARG like for any other resampled scale.
 * PD_ERR_UNSUPPORTED, naming the limit, before anything is launched: a scale of more than PD_VIT_TRAIN_MAX_TOKENS tokens per image or of
 * no whole patch, n_scales above the trainer's max_scales, n above max_images, more token rows than max_rows.  Bad arguments:
 * PD_ERR_INVALID_ARG naming the argument.  A refused call leaves a pending stash as it was. */
int pd_vit_train_forward(pd_vit_trainer *tr, const pd_vit_weights *w, const float *images, int n, int H, int W,
                         const double *scale_factors, int n_scales, const float *const *pos, float *z_out, void *stream);

/* With S a scalar function of z and g_z[n, dim] = dS/dz: writes dS/dtheta for every non-NULL member of `grads` (an overwrite, in the
 * parameter's own layout; a NULL member's launches are not issued).  The scales run one at a time in reverse call order and every weight
 * gradient is accumulated over them in that order; cls_token and pos_embed are accumulated in call order, a resampled scale through the
 * adjoint of the bicubic resampling (A = -0.75, align_corners=False, source coordinate (dst + 0.5) g / (g_target + 0.1) - 0.5 per
 * axis, taps clamped to [0, g - 1]).  Consumes the stash: PD_ERR_STATE when no forward is pending.  `w` must point to the same
 * unmodified tensors as the forward's. */
int pd_vit_train_backward(pd_vit_trainer *tr, const pd_vit_weights *w, const float *g_z, const pd_vit_weight_grads *grads, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PD_ENGINE_VIT_TRAIN_H */
