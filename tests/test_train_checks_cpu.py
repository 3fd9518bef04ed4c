"""No GPU: the gradient yardstick of the training branch (tests/train_checks.py) against the oracle, the drop-in modules' own float64
forward and the reference-generated fixture tests/golden/p_losses_grad.npz (tools/make_p_losses_grad_golden.py).

  * With its own masks the helper's forward IS the oracle's (O.denoiser_forward) and denoiser_cfgs.fp64_forward's.
  * Its autograd equals plain autograd of O.denoiser_forward at a case with no flip (forcing a function's own masks changes nothing).
  * It agrees with the reference's own ``loss.mean().backward()`` (case b3n5, pred_noise / l1 and pred_x0 / l2) within 4 x the distance
    of the helper's own float32 autograd from its float64 autograd on that case -- the rule tests/test_gpu_p_losses.py uses for
    p_losses.npz."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from denoiser_cfgs import Cfg, build_dropin, fp64_copy, fp64_forward
from oracle import pd_oracle as O
from oracle.make_golden import weight_checksum
from p_losses_cases import inputs
import train_checks as TC

NONDEFAULT = Cfg(96, 4, 200, 2, 50, 40, True, False)        # the GPU suite's non-default configuration


@pytest.fixture(scope="module")
def sd64(oracle_weights):
    return O.cast_state_dict(oracle_weights, torch.float64)


def test_forward_with_own_masks_is_the_oracles(sd64):
    inp = inputs(1)
    x, t, z = inp["x_start"].double(), inp["t"], inp["z"].double()
    out, info = TC.denoiser_forward(sd64, TC.DEFAULT_NET, x, t, z)
    assert torch.equal(out, O.denoiser_forward(sd64, x, t, z))
    assert len(info["pre"]) == 9 and info["pre"][0].shape == (3, 5, 1024) and info["pre"][8].shape == (3, 5, 128)
    again, _ = TC.denoiser_forward(sd64, TC.DEFAULT_NET, x, t, z, masks=info["masks"])
    assert torch.equal(out, again)


def test_forward_of_a_non_default_cfg_is_the_dropin_modules_fp64_forward():
    den = build_dropin(NONDEFAULT, seed=31)
    g = torch.Generator().manual_seed(3)
    x, z, t = torch.randn(3, 7, 9, generator=g), torch.randn(3, 7, NONDEFAULT.z, generator=g), torch.tensor([0, 99, 41])
    d64 = fp64_copy(den)
    sd = {k: v for k, v in d64.state_dict().items()}
    out, _ = TC.denoiser_forward(sd, TC.Net.of_cfg(NONDEFAULT), x.double(), t, z.double())
    ref = fp64_forward(d64, x, t, z)
    assert (out - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


def test_autograd_with_own_masks_is_plain_autograd_of_the_oracle(sd64):
    inp = inputs(1)
    mine = TC.loss_and_grads(sd64, TC.DEFAULT_NET, inp, "pred_noise", "l1")
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in sd64.items()}
    z = inp["z"].double().requires_grad_(True)
    tb = O.diffusion_tables(dtype=torch.float64)
    x_t = TC.q_sample(inp["x_start"].double(), inp["noise"].double(), inp["t"], tb)
    loss = (O.denoiser_forward(sd, x_t, inp["t"], z) - inp["noise"].double()).abs().mean()
    names = list(sd)
    gs = torch.autograd.grad(loss, [sd[n] for n in names] + [z])
    for n, g in zip(names + ["z"], gs):
        assert TC.grad_dist(mine["grads"][n], g) <= 1e-12, n


@pytest.mark.parametrize("objective,loss_type", TC.GOLDEN_VARIANTS)
def test_helper_agrees_with_the_reference_fixture(oracle_weights, sd64, objective, loss_type):
    gold = load_golden("p_losses_grad.npz")
    np.testing.assert_allclose(weight_checksum(oracle_weights), gold["weight_checksum"], rtol=1e-9)
    inp = inputs(int(gold["case"]))
    r64 = TC.loss_and_grads(sd64, TC.DEFAULT_NET, inp, objective, loss_type, dtype=torch.float64)
    r32 = TC.loss_and_grads(oracle_weights, TC.DEFAULT_NET, inp, objective, loss_type, dtype=torch.float32)
    assert all(torch.equal(a, b) for a, b in zip(r32["masks"], r64["masks"])) and torch.equal(r32["signs"].double(), r64["signs"])   # a case with no flip
    names = list(oracle_weights)                                       # state-dict order = named_parameters order of the reference
    assert len(names) == int(gold["n_params"])
    key = f"{objective}_{loss_type}"
    assert abs(float(gold[key + "_loss_mean"]) - r64["loss"].mean().item()) <= 4e-6 * r64["loss"].mean().item()
    worst = (0.0, 0.0, "")
    for i, n in enumerate(names):
        g64 = r64["grads"][n]
        own = TC.grad_dist(r32["grads"][n], g64)
        scale = g64.abs().max().item()
        idx = TC.sample_indices(i, g64.numel())
        vals = torch.from_numpy(gold[key + "_vals"][i]).double()
        e = (vals - g64.reshape(-1)[idx]).abs().max().item() / scale
        worst = max(worst, (e / max(own, 1e-30), e, n))
        assert e <= 4.0 * own, (n, e, own)
        assert abs(float(gold[key + "_max"][i]) - scale) <= 4.0 * own * scale, (n, "max")
        assert abs(float(gold[key + "_sum"][i]) - g64.sum().item()) <= 4.0 * own * scale * g64.numel(), (n, "sum")
    print(f"{key}: worst fixture distance / own distance = {worst[0]:.2f} ({worst[1]:.2e}, {worst[2]})")
