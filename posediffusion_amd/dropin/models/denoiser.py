"""Drop-in `Denoiser` / `TransformerEncoderWrapper` (pose_diffusion/models/denoiser.py:22-98).

Same constructor arguments, same parameter names (checkpoints load with strict=True), same
``forward(x [B,N,9], t [B], z [B,N,z_dim]) -> [B,N,9]`` -- but forward runs the hand-written HIP
kernels (posediffusion_amd/csrc/pd_denoiser.hip; pd_denoiser_generic.hip for every configuration
other than cfgs/default.yaml's) instead of ~970 ATen launches.

The configurations the engine runs (anything else raises ValueError at construction, before any GPU work):
d_model a multiple of 32 in [32, 2048]; nhead dividing it with a head dim that is a multiple of 4 in [8, 256];
dim_feedforward in [1, 8192]; 1 to 16 encoder layers; pre- or post-norm; z_dim in [1, 4096]; mlp_hidden_dim in
[1, 1024]; with or without the pivot one-hot; target_dim 9; batch_first encoders."""
from typing import Dict

import torch
import torch.nn as nn

from posediffusion_amd.compat import instantiate
from util.embedding import PoseEmbedding, TimeStepEmbedding


MAX_LAYERS = 16     # PD_MAX_LAYERS (include/pd_engine.h)


def check_trunk_cfg(d_model: int, nhead: int, num_encoder_layers: int, dim_feedforward: int, batch_first: bool = True):
    """ValueError naming the limit when the HIP engine cannot run this encoder (the ranges of include/pd_engine.h)."""
    if not batch_first:
        raise ValueError("the HIP engine implements batch_first=True encoders only")
    if d_model % 32 or not 32 <= d_model <= 2048:
        raise ValueError(f"d_model must be a multiple of 32 in [32, 2048], got {d_model}")
    if nhead < 1 or d_model % nhead:
        raise ValueError(f"nhead must divide d_model ({d_model}), got {nhead}")
    hd = d_model // nhead
    if hd % 4 or not 8 <= hd <= 256:
        raise ValueError(f"the head dim d_model / nhead must be a multiple of 4 in [8, 256], got {hd}")
    if not 1 <= dim_feedforward <= 8192:
        raise ValueError(f"dim_feedforward must be in [1, 8192], got {dim_feedforward}")
    if not 1 <= num_encoder_layers <= MAX_LAYERS:
        raise ValueError(f"num_encoder_layers must be in [1, {MAX_LAYERS}], got {num_encoder_layers}")


def TransformerEncoderWrapper(d_model: int, nhead: int, num_encoder_layers: int, dim_feedforward: int = 2048,
                              dropout: float = 0.1, norm_first: bool = True, batch_first: bool = True):
    """Weight container with nn.TransformerEncoder's parameter names (denoiser.py:79-98)."""
    check_trunk_cfg(d_model, nhead, num_encoder_layers, dim_feedforward, batch_first)
    layer = nn.TransformerEncoderLayer(d_model=d_model, nhead=nhead, dim_feedforward=dim_feedforward, dropout=dropout,
                                       batch_first=batch_first, norm_first=norm_first)
    return nn.TransformerEncoder(layer, num_encoder_layers)


class Denoiser(nn.Module):
    def __init__(self, TRANSFORMER: Dict, target_dim: int = 9, pivot_cam_onehot: bool = True, z_dim: int = 384,
                 mlp_hidden_dim: int = 128):
        super().__init__()
        if target_dim != 9:
            raise ValueError(f"the HIP engine is built for target_dim=9 (the 9-wide pose encoding), got {target_dim}")
        if not 1 <= z_dim <= 4096:
            raise ValueError(f"z_dim must be in [1, 4096], got {z_dim}")
        if not 1 <= mlp_hidden_dim <= 1024:
            raise ValueError(f"mlp_hidden_dim must be in [1, 1024], got {mlp_hidden_dim}")
        self.pivot_cam_onehot, self.target_dim = pivot_cam_onehot, target_dim
        self.time_embed = TimeStepEmbedding()
        self.pose_embed = PoseEmbedding(target_dim=target_dim)
        first_dim = self.time_embed.out_dim + self.pose_embed.out_dim + z_dim + int(pivot_cam_onehot)
        d_model = TRANSFORMER["d_model"]
        self._first = nn.Linear(first_dim, d_model)
        self._trunk = instantiate(TRANSFORMER, _recursive_=False)
        self._last = nn.Sequential(nn.Linear(d_model, mlp_hidden_dim), nn.LayerNorm(mlp_hidden_dim), nn.ReLU(inplace=True),
                                   nn.Linear(mlp_hidden_dim, target_dim))
        # older pytorch3d checkpoints carry the (non-learned) harmonic frequencies as a buffer
        self._register_load_state_dict_pre_hook(self._drop_harmonic_buffers)

    @staticmethod
    def _drop_harmonic_buffers(state_dict, prefix, *args):
        for k in [k for k in state_dict if k.startswith(prefix + "pose_embed._emb_pose.")]:
            state_dict.pop(k)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, t: torch.Tensor, z: torch.Tensor):
        from posediffusion_amd.host import get_engine
        B, N, _ = x.shape
        eng = get_engine(self, None, B, N)
        t = torch.as_tensor(t).reshape(-1)
        steps = t.unique().tolist()
        if len(steps) == 1:
            return eng.denoise(x, z, int(steps[0]))
        if t.numel() != B:
            raise ValueError(f"t must hold one timestep or one per sequence ({B}), got {t.numel()}")
        if steps[0] < 0 or steps[-1] >= eng.timesteps:          # (the engine would clamp them and flag it asynchronously)
            raise ValueError(f"timesteps must lie in [0, {eng.timesteps}), got {steps[0]} .. {steps[-1]}")
        return eng.denoise_t(x, z, t)        # per-sequence timesteps (the training branch, gaussian_diffuser.py:331): one pass
