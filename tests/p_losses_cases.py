"""The cases of tests/golden/p_losses.npz: GaussianDiffusion.p_losses (models/gaussian_diffuser.py:308-327) of the UNMODIFIED reference
with one timestep per sequence, under both objectives and both loss types.  Shared by tools/make_p_losses_golden.py (the recipe),
tests/test_p_losses_golden_cpu.py and tests/test_gpu_p_losses.py.  Inputs are not stored: they are redrawn from the seeds below."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Tuple

import numpy as np
import torch


class Case(NamedTuple):
    B: int
    N: int
    t: Tuple[int, ...]

    @property
    def name(self) -> str:
        return f"b{self.B}n{self.N}"


CASES: List[Case] = [
    Case(1, 1, (0,)),
    Case(3, 5, (0, 57, 99)),
    Case(5, 13, (99, 3, 3, 40, 0)),          # unsorted, with a repeat
    Case(2, 64, (98, 1)),
]
OBJECTIVES = ("pred_noise", "pred_x0")
LOSS_TYPES = ("l1", "l2")
SEED = 4100


def inputs(ci: int) -> Dict[str, torch.Tensor]:
    """x_start, noise [B, N, 9], z [B, N, 384] (posediffusion_amd.synth.make_z) and t [B] int64 of case ci."""
    from posediffusion_amd import synth
    c = CASES[ci]
    g = torch.Generator().manual_seed(SEED + ci)
    x_start = torch.randn(c.B, c.N, 9, generator=g)
    noise = torch.randn(c.B, c.N, 9, generator=g)
    return {"x_start": x_start, "noise": noise, "z": synth.make_z(c.B, c.N, seed=SEED + 100 * ci), "t": torch.tensor(c.t, dtype=torch.long)}


def fp64_p_losses(model_out: torch.Tensor, x_start, noise, t, objective: str, tables64: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """x_t, x_0_pred and both losses in float64 from a model output, by the schedule formulas (:211-216, :190-194, :314-323)."""
    x_start, noise, model_out = x_start.double(), noise.double(), model_out.double()
    at = lambda name: tables64[name][t].reshape(-1, 1, 1)                       # noqa: E731  (the reference's `extract`)
    x_t = at("sqrt_alphas_cumprod") * x_start + at("sqrt_one_minus_alphas_cumprod") * noise
    if objective == "pred_noise":
        target, x0 = noise, at("sqrt_recip_alphas_cumprod") * x_t - at("sqrt_recipm1_alphas_cumprod") * model_out
    else:
        target, x0 = x_start, model_out
    d = model_out - target
    return {"x_t": x_t, "x_0_pred": x0, "loss_l1": d.abs(), "loss_l2": d * d}


def make_golden(out_path: str):
    """tests/golden/p_losses.npz from the reference's own GaussianDiffusion + Denoiser in .eval(), run on CPU through oracle/ref_stubs.py
    (build container only; tools/make_p_losses_golden.py is the command).  The weights are the conftest's seeded ones (seed 0 +
    randomize_norm_and_bias_), guarded by the checksum of the other fixtures."""
    import os
    from oracle import ref_stubs as RS
    from oracle.make_golden import weight_checksum
    from posediffusion_amd import synth
    torch.set_num_threads(1)                      # bit-reproducible reference runs
    diff = RS.build_reference_diffuser(seed=0)
    synth.randomize_norm_and_bias_(diff.model)
    diff.eval()
    out = {"weight_checksum": weight_checksum(diff.model.state_dict()), "seed": np.array(SEED)}
    for ci, c in enumerate(CASES):
        inp = inputs(ci)
        out[f"{c.name}_t"] = inp["t"].numpy()
        for obj in OBJECTIVES:
            diff.objective = obj
            res = {}
            for lt in LOSS_TYPES:
                diff.loss_type = lt
                with torch.no_grad():
                    r = diff.p_losses(inp["x_start"], inp["t"], z=inp["z"], noise=inp["noise"])
                assert torch.equal(r["t"], inp["t"]) and torch.equal(r["noise"], inp["noise"])
                if res:
                    assert torch.equal(r["x_t"], res["x_t"]) and torch.equal(r["x_0_pred"], res["x_0_pred"])
                res["x_t"], res["x_0_pred"], res[f"loss_{lt}"] = r["x_t"], r["x_0_pred"], r["loss"]
            with torch.no_grad():
                res["model_out"] = diff.model(res["x_t"], inp["t"], inp["z"])
            for k, v in res.items():
                out[f"{c.name}_{obj}_{k}"] = v.numpy()
    np.savez_compressed(out_path, **out)
    print(f"wrote {out_path} ({os.path.getsize(out_path)} bytes, {len(CASES)} cases x {len(OBJECTIVES)} objectives)")
