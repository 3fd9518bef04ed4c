"""Non-default Denoiser configurations (the shape-generic denoiser path, posediffusion_amd/csrc/pd_denoiser_generic.hip): the seed
protocol that builds their weights through the drop-in modules, and the fp64 forward the GPU tests compare against.  Shared by
tests/test_denoiser_cfgs_cpu.py, tests/test_gpu_denoiser_cfgs.py, tests/test_gpu_denoiser_ranges.py and tools/make_denoiser_cfg_golden.py."""
from __future__ import annotations

import copy
from typing import Dict, NamedTuple

import numpy as np
import torch


class Cfg(NamedTuple):
    d: int
    heads: int
    ff: int
    layers: int
    z: int
    hidden: int
    norm_first: bool
    pivot: bool

    @property
    def name(self) -> str:
        return (f"d{self.d}h{self.heads}ff{self.ff}l{self.layers}z{self.z}m{self.hidden}"
                f"{'' if self.norm_first else '_post'}{'' if self.pivot else '_nopivot'}")

    def transformer(self) -> Dict:
        return {"_target_": "models.TransformerEncoderWrapper", "d_model": self.d, "nhead": self.heads, "dim_feedforward": self.ff,
                "num_encoder_layers": self.layers, "dropout": 0.1, "batch_first": True, "norm_first": self.norm_first}

    def denoiser_kwargs(self) -> Dict:
        return {"pivot_cam_onehot": self.pivot, "z_dim": self.z, "mlp_hidden_dim": self.hidden}


# the GPU suite's configurations (d, heads, ff, layers, z, hidden, norm_first, pivot)
CONFIGS = [
    Cfg(256, 8, 512, 4, 384, 128, True, True),
    Cfg(768, 12, 3072, 12, 768, 256, True, True),
    Cfg(512, 4, 1024, 8, 384, 128, False, True),
    Cfg(384, 6, 2048, 2, 2048, 64, True, False),
    Cfg(96, 3, 160, 1, 10, 20, False, False),
]
# the limits of the family and its padding boundaries (tests/test_gpu_denoiser_ranges.py): one or two axes at an edge, the rest small so
# that the fp64 forward stays cheap.  Kf = 317 + z + pivot is _first's width (padded to a multiple of 32), Dp / Fp / Hp are d / ff /
# hidden padded to a multiple of 64, head dim = d / heads (pd_gen_attn_kernel: output dims lane + 64 cc, cc = 0..3)
EDGE_CFGS = [
    Cfg(32, 4, 64, 2, 16, 32, True, True),           # smallest d (Dp = 64: 32 padding columns), head dim 8
    Cfg(96, 8, 96, 2, 35, 24, False, True),          # head dim 12; Kf = 353 = 11 x 32 + 1
    Cfg(160, 8, 65, 1, 34, 65, True, True),          # head dim 20; ff and hidden 65 (one past 64); Kf = 352 exactly
    Cfg(544, 8, 128, 1, 8, 64, True, False),         # head dim 68 (output slot 1 partly used); Dp = 576
    Cfg(256, 1, 256, 2, 64, 128, False, True),       # head dim 256 (all four output slots), one head
    Cfg(2016, 8, 64, 1, 32, 64, True, True),         # head dim 252; Dp = 2048
    Cfg(2048, 16, 64, 1, 16, 32, True, False),       # largest d
    Cfg(64, 2, 8192, 1, 16, 32, True, True),         # largest ff
    Cfg(64, 4, 1, 2, 1, 1, False, True),             # smallest ff, z and hidden (the tail's LayerNorm output is its beta)
    Cfg(64, 4, 1, 2, 1, 20, False, True),            # smallest ff and z again, visible: at hidden 1 the output does not depend on them
    Cfg(64, 4, 128, 1, 4096, 1024, True, True),      # largest z and hidden (all 16 hidden slots of pd_gen_tail_kernel)
    Cfg(64, 8, 128, 16, 32, 64, True, False),        # 16 layers (PD_MAX_LAYERS), head dim 8
]
# the configurations of tests/golden/denoiser_cfgs.npz (outputs of the reference's own models/denoiser.py)
GOLDEN_CFGS = [
    Cfg(96, 3, 160, 1, 10, 20, False, False),
    Cfg(256, 8, 512, 2, 384, 128, False, True),
    Cfg(128, 4, 200, 2, 64, 32, True, False),
]
GOLDEN_SEED = 5


def init_and_perturb_(den: torch.nn.Module, seed: int):
    """The reference init rule (pose_diffusion_model.py:67-74), then the test perturbation of every bias / LayerNorm
    (posediffusion_amd.synth.randomize_norm_and_bias_) so that a dropped bias or gamma cannot pass."""
    from posediffusion_amd import synth
    synth.reference_init_(den)
    synth.randomize_norm_and_bias_(den, seed=seed + 1234)


def build_dropin(cfg: Cfg, seed: int):
    """The drop-in Denoiser of `cfg`: torch.manual_seed(seed), construction, init + perturbation (CPU, fp32, eval)."""
    from posediffusion_amd import synth
    from posediffusion_amd.compat import AttrDict
    models = synth._dropin()
    torch.manual_seed(seed)
    den = models.Denoiser(TRANSFORMER=AttrDict(cfg.transformer()), **cfg.denoiser_kwargs())
    init_and_perturb_(den, seed)
    return den.eval()


def weight_checksum(sd: Dict[str, torch.Tensor], layers: int) -> np.ndarray:
    keys = ["_first.weight", "_trunk.layers.0.self_attn.in_proj_weight", f"_trunk.layers.{layers - 1}.linear2.weight", "_last.0.weight",
            "_last.3.weight", f"_trunk.layers.{layers - 1}.norm2.bias", "time_embed.linear.2.bias"]
    return np.array([float(sd[k].double().abs().sum()) for k in keys])


def fp64_copy(den: torch.nn.Module) -> torch.nn.Module:
    """A float64 CPU copy of `den` for fp64_forward (which otherwise copies `den` on every call)."""
    return copy.deepcopy(den).cpu().double().eval()


def is_fp64_copy(den: torch.nn.Module) -> bool:
    p = den._first.weight
    return p.dtype == torch.float64 and p.device.type == "cpu" and not den.training


@torch.no_grad()
def fp64_forward(den: torch.nn.Module, x: torch.Tensor, t: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """Denoiser.forward in float64: the drop-in's own nn modules (_first, nn.TransformerEncoder, _last) cast to float64, with the
    oracle's harmonic and time embedding (models/denoiser.py:53-76)."""
    from oracle import pd_oracle as O
    d64 = den if is_fp64_copy(den) else fp64_copy(den)
    sd = {k: v for k, v in d64.state_dict().items()}
    x, z = x.detach().cpu().double(), z.detach().cpu().double()
    B, N, _ = x.shape
    t_emb = O.timestep_embedding(torch.as_tensor(t).reshape(-1).expand(B).cpu(), sd)[:, None, :].expand(-1, N, -1)
    parts = [O.harmonic_embedding(x), t_emb, z]
    if den.pivot_cam_onehot:
        pivot = torch.zeros_like(z[..., :1])
        pivot[:, 0] = 1.0
        parts.append(pivot)
    h = d64._first(torch.cat(parts, dim=-1))
    h = d64._trunk(h)
    return d64._last(h)


GOLDEN_SHAPES = {"b2n5": (2, 5), "b1n1": (1, 1), "b3n9": (3, 9)}
GOLDEN_STEPS = (99, 3)


def make_golden(out_path: str):
    """tests/golden/denoiser_cfgs.npz from the UNMODIFIED reference models/denoiser.py, run on CPU through oracle/ref_stubs.py
    (build container only; tools/make_denoiser_cfg_golden.py is the command).  For every GOLDEN_CFGS entry the reference's own
    Denoiser is built with the seed protocol of build_dropin (the drop-in is asserted to draw the same weights) and its forward is
    recorded at two timesteps.  Weights are not stored, only their checksum."""
    import os
    from oracle import ref_stubs as RS
    from posediffusion_amd import synth
    from posediffusion_amd.compat import AttrDict
    torch.set_num_threads(1)                      # bit-reproducible reference runs
    ref = RS.load_reference()
    cases = {}
    for ci, cfg in enumerate(GOLDEN_CFGS):
        seed = GOLDEN_SEED + ci
        torch.manual_seed(seed)
        den = ref.Denoiser(TRANSFORMER=AttrDict(cfg.transformer()), **cfg.denoiser_kwargs())
        init_and_perturb_(den, seed)
        den.eval()
        sd = den.state_dict()
        mine = build_dropin(cfg, seed).state_dict()
        assert list(sd) == list(mine) and all(torch.equal(sd[k], mine[k]) for k in sd), cfg   # the drop-in draws the same weights
        cases[f"c{ci}_cfg"] = np.array([cfg.d, cfg.heads, cfg.ff, cfg.layers, cfg.z, cfg.hidden, int(cfg.norm_first), int(cfg.pivot), seed])
        cases[f"c{ci}_weight_checksum"] = weight_checksum(sd, cfg.layers)
        g = torch.Generator().manual_seed(100 + ci)
        for name, (B, N) in GOLDEN_SHAPES.items():
            x = torch.randn(B, N, 9, generator=g)
            z = synth.make_z(B, N, seed=300 + ci, z_dim=cfg.z)
            cases[f"c{ci}_{name}_x"], cases[f"c{ci}_{name}_z"] = x.numpy(), z.numpy()
            for t in GOLDEN_STEPS:
                with torch.no_grad():
                    cases[f"c{ci}_{name}_eps_t{t}"] = den(x, torch.full((B,), t, dtype=torch.long), z).numpy()
    np.savez_compressed(out_path, **cases)
    print(f"wrote {out_path} ({os.path.getsize(out_path)} bytes, {len(GOLDEN_CFGS)} configurations)")
