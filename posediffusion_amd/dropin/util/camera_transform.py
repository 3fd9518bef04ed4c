"""pose_encoding_to_camera and camera_to_pose_encoding (pose_diffusion/util/camera_transform.py:64-129) on the HIP engine.
``pose_encoding_to_camera`` is differentiable like the reference's: with grad mode on and an input that requires grad (the
``x_0_pred`` of ``GaussianDiffusion.engine_grad_outputs``) R, T and focal_length carry grad, the backward being
pd_pose_to_camera_backward (include/pd_engine_train.h); otherwise it is the plain decode, no grad."""
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
