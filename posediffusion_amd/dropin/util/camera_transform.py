"""pose_encoding_to_camera and camera_to_pose_encoding (pose_diffusion/util/camera_transform.py:64-129) on the HIP engine.
``pose_encoding_to_camera`` is differentiable like the reference's: with grad mode on and an input that requires grad (the
``x_0_pred`` of ``GaussianDiffusion.engine_grad_outputs``) R, T and focal_length carry grad, the backward being
pd_pose_to_camera_backward (include/pd_engine_train.h); otherwise it is the plain decode, no grad.

The intrinsics helpers of the reference's datasets (camera_transform.py:14-61: ``bbox_xyxy_to_xywh``, ``adjust_camera_to_bbox_crop_``,
``adjust_camera_to_image_scale_`` and the two NDC / pixel conversions) are here as well, as plain device-agnostic torch / numpy: they
run once per image inside dataset workers on CPU tensors of two elements, where a kernel launch would be the wrong tool."""
import numpy as np
import torch

from posediffusion_amd import _lib
from posediffusion_amd.compat import PerspectiveCameras


def pose_encoding_to_camera(pose_encoding, pose_encoding_type="absT_quaR_logFL", log_focal_length_bias=1.8,
                            min_focal_length=0.1, max_focal_length=20, return_dict=False, engine=None):
    if pose_encoding_type != "absT_quaR_logFL":
        raise ValueError(f"Unknown pose encoding {pose_encoding_type}")           # camera_transform.py:98-99
    if engine is None:
        from posediffusion_amd.host import current_engine
        engine = current_engine(pose_encoding.device)
    if torch.is_grad_enabled() and getattr(pose_encoding, "requires_grad", False):
        from posediffusion_amd.train import pose_to_camera_with_grad
        R, T, f = pose_to_camera_with_grad(engine, pose_encoding, log_focal_length_bias, min_focal_length, max_focal_length)
    else:
        with torch.no_grad():
            R, T, f = engine.pose_to_camera(pose_encoding, log_focal_length_bias, min_focal_length, max_focal_length)
    if return_dict:
        return {"focal_length": f, "R": R, "T": T}
    return PerspectiveCameras(focal_length=f, R=R, T=T, device=R.device)


@torch.no_grad()
def camera_to_pose_encoding(camera, pose_encoding_type="absT_quaR_logFL", log_focal_length_bias=1.8, min_focal_length=0.1,
                            max_focal_length=20, engine=None):
    """[T | matrix_to_quaternion(R) | log(clamp(focal_length)) - bias] of ``camera`` (.R [.., 3, 3], .T [.., 3], .focal_length [.., 2]),
    shape [n, 9] (camera_transform.py:108-129); the quaternion rule is current pytorch3d's (include/pd_engine.h pd_camera_to_pose)."""
    if pose_encoding_type != "absT_quaR_logFL":
        raise ValueError(f"Unknown pose encoding {pose_encoding_type}")           # camera_transform.py:126-127
    if engine is None:
        from posediffusion_amd.host import current_engine
        engine = current_engine(camera.R.device)
    return engine.camera_to_pose(camera.R, camera.T, camera.focal_length, log_focal_length_bias, min_focal_length, max_focal_length)


def bbox_xyxy_to_xywh(xyxy):
    """(x0, y0, x1, y1) -> (x0, y0, width, height), numpy (camera_transform.py:14-17)."""
    return np.concatenate([xyxy[:2], xyxy[2:] - xyxy[:2]])


def _convert_ndc_to_pixels(focal_length: torch.Tensor, principal_point: torch.Tensor, image_size_wh: torch.Tensor):
    """PyTorch3D NDC intrinsics -> pixels: the NDC unit is half the SHORTER image side (camera_transform.py:46-51)."""
    half_wh = image_size_wh / 2
    unit = half_wh.min()
    return focal_length * unit, half_wh - principal_point * unit


def _convert_pixels_to_ndc(focal_length_px: torch.Tensor, principal_point_px: torch.Tensor, image_size_wh: torch.Tensor):
    """Pixel intrinsics -> PyTorch3D NDC of an image of ``image_size_wh`` (camera_transform.py:54-61)."""
    half_wh = image_size_wh / 2
    unit = half_wh.min()
    return focal_length_px / unit, (half_wh - principal_point_px) / unit


def adjust_camera_to_bbox_crop_(fl, pp, image_size_wh: torch.Tensor, clamp_bbox_xywh: torch.Tensor):
    """NDC intrinsics of the crop ``clamp_bbox_xywh`` of an image of ``image_size_wh`` (camera_transform.py:20-28): the principal point
    moves by the crop's corner in pixels, the NDC unit becomes that of the crop."""
    fl_px, pp_px = _convert_ndc_to_pixels(fl, pp, image_size_wh)
    return _convert_pixels_to_ndc(fl_px, pp_px - clamp_bbox_xywh[:2], clamp_bbox_xywh[2:])


def adjust_camera_to_image_scale_(fl, pp, original_size_wh: torch.Tensor, new_size_wh: torch.LongTensor):
    """NDC intrinsics after resizing the image to ``new_size_wh`` (camera_transform.py:31-43): pixels scale by the SMALLER of the two
    size ratios."""
    fl_px, pp_px = _convert_ndc_to_pixels(fl, pp, original_size_wh)
    new_wh = new_size_wh.float()
    ratio = (new_wh / original_size_wh).min(dim=-1, keepdim=True).values
    return _convert_pixels_to_ndc(fl_px * ratio, pp_px * ratio, new_wh)
