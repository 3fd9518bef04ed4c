"""Drop-in ``util.normalize_cameras`` (pose_diffusion/util/normalize_cameras.py:52-148) on the HIP engine: the reference's names and
signatures on the project's ``PerspectiveCameras``, each ONE launch of pd_normalize_cameras (include/pd_engine_cameras.h) on device
tensors, without pytorch3d.  Every function returns a NEW camera object with ``focal_length`` and ``principal_point`` carried over.

Where the reference's ``lstsq`` would return a minimum-norm point for axes that determine none (all parallel, a single frame), and
where it raises ``ValueError("p_intersect is NaN")``, these raise ``ValueError`` naming the reason.

Extension: ``normalize_cameras_batch(cameras, batch_size=, n_frames=, ...)`` for B x N cameras held in one object, as train.py holds
them.  The reference's ``intersect_skew_line_groups``, ``intersect_skew_lines_high_dim`` and ``_point_line_distance`` are not needed."""
import torch

from posediffusion_amd import cameras as _cam
from posediffusion_amd.compat import PerspectiveCameras


def _like(cameras, R, T):
    n = R.shape[0] * R.shape[1]
    return PerspectiveCameras(focal_length=cameras.focal_length, principal_point=cameras.principal_point, R=R.reshape(n, 3, 3),
                              T=T.reshape(n, 3), device=R.device)


def normalize_cameras_batch(cameras, batch_size=None, n_frames=None, compute_optical=True, first_camera=True, rotation_only=False,
                            normalize_T=False, on_degenerate="raise", return_result=False):
    """``normalize_cameras`` for ``batch_size`` sequences of ``len(cameras) / batch_size`` cameras each (``n_frames`` [B]: the real
    frames of a padded batch; padding cameras come back as zeros).  ``return_result=True``: also the engine's result object
    (``p_intersect``, ``scale``, ``status``; posediffusion_amd.cameras.NormalizedCameras)."""
    res = _cam.normalize_cameras_batch(cameras.R, cameras.T, n_frames, compute_optical=compute_optical, first_camera=first_camera,
                                       rotation_only=rotation_only, normalize_T=normalize_T, on_degenerate=on_degenerate,
                                       batch_size=batch_size)
    new_cameras = _like(cameras, res.R, res.T)
    return (new_cameras, res) if return_result else new_cameras


def normalize_cameras(cameras, compute_optical=True, first_camera=True, scale=1.0, normalize_T=False):
    """normalize_cameras.py:75-114 (``scale`` is unused there as well: it is overwritten before it is read)."""
    return normalize_cameras_batch(cameras, compute_optical=bool(compute_optical), first_camera=first_camera, normalize_T=normalize_T)


def first_camera_transform(cameras, rotation_only=False):
    """normalize_cameras.py:132-148: express every camera in camera 0's frame."""
    return normalize_cameras_batch(cameras, compute_optical=None, first_camera=True, rotation_only=rotation_only)


def normalize_Trans(new_cameras):
    """normalize_cameras.py:118-128: T / clamp(||T[1:]||_F / sqrt(N - 1) / 2, 0.01, 100); one camera is returned unchanged."""
    return normalize_cameras_batch(new_cameras, compute_optical=None, first_camera=False, normalize_T=True)


def compute_optical_axis_intersection(cameras):
    """normalize_cameras.py:52-72 -> (p_intersect [1, 3], dist [1, 1, N], p_line_intersect [1, 1, N, 3], pp2 [N, 3], r [1, 1, N, 3]).
    The first three and ``r`` come from the launch; ``pp2`` (the principal points unprojected at depth 1, = camera centre + third column
    of R, which only the reference's own callers of this function read) is formed from R and T by three tensor operations."""
    res = _cam.normalize_cameras_batch(cameras.R, cameras.T, compute_optical=True, first_camera=False, diagnostics=True)
    n = res.R.shape[1]
    R, T = cameras.R.to(torch.float32), cameras.T.to(torch.float32)
    centers = -(R @ T[:, :, None])[:, :, 0]
    pp2 = centers + R[:, :, 2]
    return res.p_intersect, res.dist.reshape(1, 1, n), res.foot.reshape(1, 1, n, 3), pp2, res.axis.reshape(1, 1, n, 3)
