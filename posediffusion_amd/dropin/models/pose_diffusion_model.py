"""Drop-in `PoseDiffusionModel` (pose_diffusion/models/pose_diffusion_model.py:35-142).

``forward(image, gt_cameras=None, sequence_name=None, cond_fn=None, cond_start_step=0, training=True,
batch_repeat=-1)`` keeps the reference signature; `training=False` returns
``{"pred_cameras": PerspectiveCameras(R, T, focal_length) in PyTorch3D NDC, "z": features}``.
`training=True` (with ``gt_cameras``) follows :111-126: the diffusion results of ``GaussianDiffusion.forward`` on the encoded cameras plus
``pred_cameras`` decoded from ``x_0_pred`` -- by default the forward half only: eval-mode network, no grad (dropin/models/gaussian_diffuser.py).
With ``diffuser.engine_grad`` and ``diffuser.engine_grad_outputs`` set, ``x_0_pred`` carries grad and so do ``pred_cameras.R``, ``.T`` and
``.focal_length`` (the decode's backward is pd_pose_to_camera_backward): a camera-space term added to the total reaches the denoiser and,
through dz, the backbone.
Extensions: ``z=`` accepts precomputed image features instead of ``image`` (skips the feature extractor).  ``n_frames=`` [B] (training
branch): frame counts of a padded batch, handed to the diffuser -- ``gt_cameras`` still holds B x N cameras, the padding entries being any
valid camera; their ``pred_cameras`` entries carry no meaning, and ``loss`` is +0 there (mean over real frames:
``loss.sum() / (9 * sum(n_frames))``).  ``normalize_gt=`` (training branch; default None = off): a dict of the reference's
``normalize_cameras`` keywords (``compute_optical``, ``first_camera``, ``normalize_T``; ``{}`` = its defaults) -- ``gt_cameras`` are then
the RAW cameras: they are normalised per sequence (``n_frames`` honoured) and encoded by one launch of pd_normalize_cameras
(include/pd_engine_cameras.h) in place of the ``camera_to_pose_encoding`` call, with bitwise the result of normalising them beforehand.
The encoding's padding rows are +0 there.  The dict may also hold ``on_degenerate``: by default ("raise") every call reads the
per-sequence status back -- one small device-to-host copy that synchronises the step -- and raises ``ValueError`` for a sequence that
cannot be normalised; ``{"on_degenerate": "status"}`` skips the read-back and trains on such a sequence's cameras as given."""
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from posediffusion_amd import host
from posediffusion_amd.compat import instantiate
from util.camera_transform import camera_to_pose_encoding, pose_encoding_to_camera


class PoseDiffusionModel(nn.Module):
    def __init__(self, pose_encoding_type: str, IMAGE_FEATURE_EXTRACTOR: Dict, DIFFUSER: Dict, DENOISER: Dict):
        super().__init__()
        self.pose_encoding_type = pose_encoding_type
        self.image_feature_extractor = instantiate(IMAGE_FEATURE_EXTRACTOR, _recursive_=False)
        self.diffuser = instantiate(DIFFUSER, _recursive_=False)
        denoiser = instantiate(DENOISER, _recursive_=False)
        self.diffuser.model = denoiser
        self.target_dim = denoiser.target_dim
        self.apply(self._init_weights)

    def _init_weights(self, m):
        # same rule as pose_diffusion_model.py:67-74
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def _normalized_gt_encoding(self, gt_cameras, n_seq, n_frames, batch_repeat, normalize_gt):
        """Pose encoding of ``gt_cameras`` normalised per sequence: one launch of pd_normalize_cameras with the encoder fused in."""
        if self.pose_encoding_type != "absT_quaR_logFL":
            raise ValueError(f"Unknown pose encoding {self.pose_encoding_type}")
        from posediffusion_amd.cameras import normalize_cameras_batch
        kw = dict(normalize_gt)
        unknown = set(kw) - {"compute_optical", "first_camera", "rotation_only", "normalize_T", "scale", "on_degenerate"}
        if unknown:
            raise TypeError(f"normalize_gt: unknown normalize_cameras keywords {sorted(unknown)}")
        kw.pop("scale", None)                                           # dead in the reference as well
        if "compute_optical" in kw:
            kw["compute_optical"] = bool(kw["compute_optical"])
        if n_frames is not None and batch_repeat > 0:
            n_frames = [int(v) for v in (n_frames.tolist() if hasattr(n_frames, "tolist") else n_frames)] * batch_repeat
        res = normalize_cameras_batch(gt_cameras.R, gt_cameras.T, n_frames, focal_length=gt_cameras.focal_length, batch_size=n_seq, **kw)
        return res.pose_encoding

    def forward(self, image: torch.Tensor = None, gt_cameras=None, sequence_name: Optional[List[str]] = None, cond_fn=None,
                cond_start_step=0, training=True, batch_repeat=-1, z: Optional[torch.Tensor] = None, n_frames=None, normalize_gt=None):
        if normalize_gt is not None and not training:
            raise ValueError("normalize_gt applies to the training branch (it normalises gt_cameras); call with training=True")
        if training and gt_cameras is None:
            raise NotImplementedError("the training branch needs ground-truth cameras (gt_cameras): it computes the diffusion loss of their "
                                      "pose encoding; call with training=False to sample")
        if z is None:
            B, N = image.shape[0], image.shape[1]
            z = self.image_feature_extractor(image.reshape(B * N, *image.shape[2:])).reshape(B, N, -1)
        B, N, _ = z.shape
        if training:                                                   # pose_diffusion_model.py:111-126
            eng = host.get_engine(self.diffuser.model, self.diffuser, B * max(batch_repeat, 1), N)
            if normalize_gt is None:
                pose_encoding = camera_to_pose_encoding(gt_cameras, pose_encoding_type=self.pose_encoding_type, engine=eng)
            else:
                pose_encoding = self._normalized_gt_encoding(gt_cameras, B * max(batch_repeat, 1), n_frames, batch_repeat, normalize_gt)
            if batch_repeat > 0:
                pose_encoding = pose_encoding.reshape(B * batch_repeat, -1, self.target_dim)
                z = z.repeat(batch_repeat, 1, 1)
                if n_frames is not None:
                    n_frames = [int(v) for v in (n_frames.tolist() if hasattr(n_frames, "tolist") else n_frames)] * batch_repeat
            else:
                pose_encoding = pose_encoding.reshape(B, -1, self.target_dim)
            diffusion_results = self.diffuser(pose_encoding, z=z) if n_frames is None else self.diffuser(pose_encoding, z=z, n_frames=n_frames)
            diffusion_results["pred_cameras"] = pose_encoding_to_camera(diffusion_results["x_0_pred"],
                                                                        pose_encoding_type=self.pose_encoding_type, engine=eng)
            return diffusion_results
        pose_encoding, _ = self.diffuser.sample(shape=[B, N, self.target_dim], z=z, cond_fn=cond_fn,
                                                cond_start_step=cond_start_step)
        eng = host.get_engine(self.diffuser.model, self.diffuser, B, N)
        pred_cameras = pose_encoding_to_camera(pose_encoding, pose_encoding_type=self.pose_encoding_type, engine=eng)
        return {"pred_cameras": pred_cameras, "z": z, "pose_encoding": pose_encoding}
