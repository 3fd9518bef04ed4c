/*
 * pd_engine_cameras.h -- ground-truth camera normalisation (the reference's util/normalize_cameras.py:15-148: the optical-axis
 * intersection, normalize_cameras, first_camera_transform, normalize_Trans) on one hand-written gfx950 kernel
 * (csrc/pd_cameras.hip), batched over sequences, ragged, with the pose encoding of the result fused in.
 *
 * An extension header like pd_engine_ingest.h: the function list of pd_engine.h is pinned.  The entry is stateless like the metric
 * kernels: DEVICE fp32 pointers borrowed for the call, `stream` a hipStream_t as void *, no allocation, no host synchronisation.
 * Conventions are those of pd_engine.h (return codes, pd_last_error).
 *
 * PyTorch3D row convention, X_view = X_world R + T; R row-major.  For the n real frames of one sequence:
 *   optical-axis intersection   C_i = -T_i R_i^T;  r_i = third column of R_i, l2-normalised (the reference unprojects the principal
 *       point at depth 1: the view-space point is (0, 0, 1) whatever the intrinsics);  A = sum_i (I - r_i r_i^T),
 *       b = sum_i (I - r_i r_i^T) C_i,  p = A^-1 b;  dist_i = |p - C_i|;  foot point C_i + ((p - C_i) . r_i) r_i.
 *   scale_mode 1   divisor = dist_0.  divisor == 0 exactly: T_i /= sqrt(||T||_F), R unchanged (status 1, normalize_cameras.py:95-98);
 *       otherwise T_i <- (p R_i + T_i) / divisor, R unchanged (:100-102).
 *   scale_mode 2   T_i /= sqrt(||T||_F) (:104-106).     scale_mode 0: nothing.
 *   first_camera   with R_0, T_0 the values after the scaling: R_i <- R_0^T R_i, T_i <- T_i - T_0 R_i (the new R_i); mode 2 (rotation
 *       only) leaves T_i alone.  Camera 0 becomes (I, 0).
 *   normalize_T    s = clamp(||T[1:]||_F / sqrt(n - 1) / 2, 0.01, 100), T /= s (:118-128).  With ONE real frame the reference divides
 *       0 by 0; here no division is applied (s = 1).
 * All sums (the six of A, the three of b, ||T||_F^2, ||T[1:]||_F^2) and all per-frame arithmetic are fp64, in an order that depends on
 * the sequence's frame count alone; every output value is rounded to fp32 once.
 */
#ifndef PD_ENGINE_CAMERAS_H
#define PD_ENGINE_CAMERAS_H

#include "pd_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int scale_mode;     /* 0 none, 1 optical-axis intersection, 2 sqrt(||T||_F) */
    int first_camera;   /* 0 off, 1 full, 2 rotation only */
    int normalize_T;    /* 0 / 1 */
} pd_cam_norm_cfg;

/* status_out values: the outputs of a sequence are defined under every one of them */
#define PD_CAM_OK 0            /* normalised */
#define PD_CAM_ZERO_SCALE 1    /* scale_mode 1 met dist_0 == 0 and divided T by sqrt(||T||_F) (the reference's "degenerate case"); normalised */
#define PD_CAM_RANK 2          /* scale_mode 1: the axes do not determine a point (A rank-deficient: all axes parallel, or one frame) */
#define PD_CAM_NON_FINITE 3    /* inf / NaN among the real frames' R, T, in the sums (an R whose third column is zero has no axis;
                                  ||T||_F^2 overflowing) or in p; or ||T||_F == 0 where T is divided by its root */
#define PD_CAM_BAD_COUNT 4     /* n_frames[b] outside [1, N] */

/* R [B, N, 9], T [B, N, 3].  n_frames (DEVICE int32 [B], may be NULL = N frames each): sequence b has n_frames[b] real frames in rows
 * 0 .. of its block; rows at or beyond the count are never read and are +0 in every output.  R_out / T_out may be R / T (in place).
 * Optional outputs (NULL = not wanted):
 *   enc_out [B, N, 9]   bitwise pd_camera_to_pose(R_out, T_out, focal [B, N, 2], the three focal-length parameters); needs focal;
 *   p_intersect_out [B, 3], scale_out [B]   p and the divisor the scaling stage applied (dist_0, sqrt(||T||_F), or 1 where nothing
 *       was divided; the s of normalize_T is not part of it);
 *   dist_out [B, N], foot_out [B, N, 3], axis_out [B, N, 3]   dist_i, the foot points and r_i of the INPUT cameras.
 *   p, dist, foot and axis are computed under scale_mode 1 with status 0 or 1, and are +0 otherwise.
 * status_out [B] (required), see PD_CAM_*.  Status 2 and 3: R_out, T_out are the inputs copied unchanged, scale 1.  Status 4: every
 * row of every output of the sequence is +0, nothing out of bounds is touched.  The counts live on the device, so a bad count is
 * never known on the host and is always reported as status 4.
 * Rank rule of status 2: A is factorised by an fp64 Cholesky; the sequence is refused when its smallest pivot is not above
 * 1e-10 trace(A).  (trace(A) = 2 n; two axes an angle t apart give a smallest pivot of about t^2 / 2, so the rule solves axes down to
 * 3e-5 rad apart -- 1e-3 rad gives 1.2e-7 of the trace -- and refuses what fp32 rotations cannot tell from parallel: their
 * directions carry 6e-8 of rounding, a pivot of 1e-14 of the trace.)
 * PD_ERR_INVALID_ARG naming the argument, before anything is launched: NULL R, T, cfg, R_out, T_out or status_out, B < 0, N < 1,
 * enc_out without focal, a mode outside its range.  B == 0 is a no-op. */
int pd_normalize_cameras(const float *R, const float *T, int B, int N, const int32_t *n_frames, const pd_cam_norm_cfg *cfg,
                         float *R_out, float *T_out, const float *focal, float log_focal_length_bias, float min_focal_length,
                         float max_focal_length, float *enc_out, float *p_intersect_out, float *scale_out, float *dist_out,
                         float *foot_out, float *axis_out, int32_t *status_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PD_ENGINE_CAMERAS_H */
