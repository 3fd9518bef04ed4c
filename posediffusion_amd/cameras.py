"""Ground-truth camera normalisation on the engine (include/pd_engine_cameras.h): the reference's
``util/normalize_cameras.py`` -- optical-axis intersection, ``normalize_cameras``, ``first_camera_transform``, ``normalize_Trans`` -- for
B sequences of up to N frames in ONE launch of pd_normalize_cameras, with the pose encoding of the result fused in.

``normalize_cameras_batch`` is the public entry; the reference-named functions of ``dropin/util/normalize_cameras.py`` and
``PoseDiffusionModel.forward(normalize_gt=...)`` are thin callers of it.  There is no CPU path and no fallback."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib

STATUS_REASONS = {
    _lib.PD_CAM_RANK: "the optical axes do not determine a point (all parallel, or a single frame)",
    _lib.PD_CAM_NON_FINITE: "non-finite R, T, sums (an R without an optical axis) or intersection point, or a zero translation norm to divide by",
    _lib.PD_CAM_BAD_COUNT: "frame count outside [1, N]",
}


class NormalizedCameras:
    """What one call returns: ``R`` [B, N, 3, 3], ``T`` [B, N, 3], ``pose_encoding`` [B, N, 9] (None without ``focal_length``),
    ``p_intersect`` [B, 3], ``scale`` [B] (the divisor the scaling stage applied), ``status`` [B] int32 (0 normalised, 1 the
    reference's zero-scale branch, 2 rank-deficient, 3 non-finite, 4 bad frame count); with ``diagnostics=True`` also ``dist`` [B, N],
    ``foot`` [B, N, 3] and ``axis`` [B, N, 3] of the input cameras."""
    __slots__ = ("R", "T", "pose_encoding", "p_intersect", "scale", "status", "dist", "foot", "axis")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _f32(t: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"normalize_cameras_batch: {what} must be a torch.Tensor (got {type(t).__name__})")
    if t.device.type != "cuda":
        raise RuntimeError(f"normalize_cameras_batch: {what} is on {t.device}; the engine needs tensors on an AMD GPU "
                           "(there is no CPU fallback)")
    return t.detach().to(torch.float32).contiguous()


def normalize_cameras_batch(R, T, n_frames=None, *, compute_optical: Optional[bool] = True, first_camera=True, rotation_only=False,
                            normalize_T=False, focal_length=None, log_focal_length_bias=1.8, min_focal_length=0.1,
                            max_focal_length=20, out=None, on_degenerate="raise", batch_size=None,
                            diagnostics=False) -> NormalizedCameras:
    """Normalise B sequences of cameras (PyTorch3D row convention, ``X_view = X_world R + T``) in one launch on the current stream.

    ``R`` is [B, N, 3, 3] with ``T`` [B, N, 3], or [B*N, 3, 3] with ``T`` [B*N, 3] and ``batch_size=B`` (default 1 sequence).
    ``n_frames`` [B]: frame counts of a padded batch; rows beyond a count are never read and come back +0.  An int32 tensor on the
    device is used as it is; a list or a host tensor is copied to the device first, a pageable copy that blocks the host.
    ``compute_optical``: True -- translate the optical axes' intersection to the origin and make camera 0's distance to it 1; False --
    divide T by sqrt(||T||_F); None -- no scaling (what ``first_camera_transform`` and ``normalize_Trans`` alone need).
    ``first_camera`` / ``rotation_only`` / ``normalize_T``: the reference's ``first_camera_transform`` and ``normalize_Trans``.
    ``focal_length`` [B, N, 2] (or [B*N, 2]): also return ``pose_encoding``, bitwise ``camera_to_pose_encoding`` of the result.
    ``out=(R, T)``: contiguous float32 tensors to write into; they may be the inputs themselves.
    ``on_degenerate``: "raise" reads ``status`` back (one small device-to-host copy) and raises ``ValueError`` naming the sequences with
    status >= 2; "status" adds no synchronisation (none at all with device tensors throughout) and leaves ``status`` to the caller."""
    if on_degenerate not in ("raise", "status"):
        raise ValueError(f"on_degenerate must be 'raise' or 'status' (got {on_degenerate!r})")
    R32, T32 = _f32(R, "R"), _f32(T, "T")
    dev = R32.device
    if R32.dim() == 4 and tuple(R32.shape[2:]) == (3, 3):
        B, N = R32.shape[0], R32.shape[1]
    elif R32.dim() == 3 and tuple(R32.shape[1:]) == (3, 3):
        B = 1 if batch_size is None else int(batch_size)
        if B < 1 or R32.shape[0] % B:
            raise ValueError(f"batch_size = {batch_size} does not divide the {R32.shape[0]} cameras of R")
        N = R32.shape[0] // B
    else:
        raise ValueError(f"R must be [B, N, 3, 3] or [B*N, 3, 3] (got {tuple(R32.shape)})")
    if N < 1:
        raise ValueError("normalize_cameras_batch: no frames")
    if T32.device != dev or T32.numel() != B * N * 3:
        raise ValueError(f"T must hold 3 values for each of the {B} x {N} cameras of R on {dev} (got {tuple(T32.shape)} on {T32.device})")
    nf = None
    if n_frames is not None:
        nf = torch.as_tensor(n_frames).to(device=dev, dtype=torch.int32).contiguous()
        if nf.numel() != B:
            raise ValueError(f"n_frames must hold one count per sequence ({B}), got {nf.numel()}")
    F32 = None
    if focal_length is not None:
        F32 = _f32(focal_length, "focal_length")
        if F32.device != dev or F32.numel() != B * N * 2:
            raise ValueError(f"focal_length must hold 2 values for each of the {B} x {N} cameras (got {tuple(F32.shape)})")
    if out is not None:
        Ro, To = out
        for t, name, numel in ((Ro, "out[0]", B * N * 9), (To, "out[1]", B * N * 3)):
            if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != numel:
                raise ValueError(f"{name} must be a contiguous float32 tensor of {numel} values on {dev}")
    else:
        Ro, To = torch.empty(B, N, 3, 3, device=dev), torch.empty(B, N, 3, device=dev)
    cfg = _lib.pd_cam_norm_cfg(1 if compute_optical else (0 if compute_optical is None else 2),
                               0 if not first_camera else (2 if rotation_only else 1), 1 if normalize_T else 0)
    enc = torch.empty(B, N, 9, device=dev) if F32 is not None else None
    p, scale = torch.empty(B, 3, device=dev), torch.empty(B, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    dist = foot = axis = None
    if diagnostics:
        dist, foot, axis = torch.empty(B, N, device=dev), torch.empty(B, N, 3, device=dev), torch.empty(B, N, 3, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.pd_normalize_cameras(R32.data_ptr(), T32.data_ptr(), B, N, ptr(nf), C.byref(cfg), Ro.data_ptr(), To.data_ptr(),
                                            ptr(F32), float(log_focal_length_bias), float(min_focal_length), float(max_focal_length),
                                            ptr(enc), p.data_ptr(), scale.data_ptr(), ptr(dist), ptr(foot), ptr(axis), status.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream), "pd_normalize_cameras")
    if on_degenerate == "raise":
        st = status.cpu().tolist()
        bad = [(b, s) for b, s in enumerate(st) if s >= _lib.PD_CAM_RANK]
        if bad:
            raise ValueError("normalize_cameras: " + "; ".join(f"sequence {b}: {STATUS_REASONS.get(s, f'status {s}')} (status {s})"
                                                               for b, s in bad))
    return NormalizedCameras(R=Ro.view(B, N, 3, 3), T=To.view(B, N, 3), pose_encoding=enc, p_intersect=p, scale=scale, status=status,
                             dist=dist, foot=foot, axis=axis)
