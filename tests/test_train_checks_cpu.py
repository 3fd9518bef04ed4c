"""No GPU: the gradient yardstick of the training branch (tests/train_checks.py) against the oracle, the drop-in modules' own float64
forward and the reference-generated fixture tests/golden/p_losses_grad.npz (tools/make_p_losses_grad_golden.py).

  * With its own masks the helper's forward IS the oracle's (O.denoiser_forward) and denoiser_cfgs.fp64_forward's.
  * Its autograd equals plain autograd of O.denoiser_forward at a case with no flip (forcing a function's own masks changes nothing).
  * The same with a non-uniform ``g_loss`` (TC.draw_g_loss): plain autograd of sum(g |O.denoiser_forward - noise|); a ``g_loss`` read
    per row instead of per element lands far outside the 4 x own bound of tests/test_gpu_train_grad_edges.py.
  * The block helper (TC.grad_blocks / block_misses) binds a sub-block that the tensor-level maximum norm does not.
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


def test_autograd_with_a_non_uniform_g_loss_is_plain_autograd_of_the_oracle(sd64):
    inp = inputs(1)
    B, N, _ = inp["x_start"].shape
    g_loss = TC.draw_g_loss(B, N)
    nz = g_loss[g_loss != 0].abs()
    assert (g_loss[0] == 0).all() and (g_loss[:, 1] == 0).all() and (g_loss < 0).any() and (g_loss > 0).any() and nz.max() / nz.min() > 1e3
    mine = TC.loss_and_grads(sd64, TC.DEFAULT_NET, inp, "pred_noise", "l1", g_loss=g_loss)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in sd64.items()}
    z = inp["z"].double().requires_grad_(True)
    tb = O.diffusion_tables(dtype=torch.float64)
    x_t = TC.q_sample(inp["x_start"].double(), inp["noise"].double(), inp["t"], tb)
    loss = (g_loss.double() * (O.denoiser_forward(sd, x_t, inp["t"], z) - inp["noise"].double()).abs()).sum()
    names = list(sd)
    gs = torch.autograd.grad(loss, [sd[n] for n in names] + [z])
    for n, g in zip(names + ["z"], gs):
        assert TC.grad_dist(mine["grads"][n], g) <= 1e-12, n
    assert mine["grads"]["z"][0].abs().max().item() == 0.0          # a sequence whose g_loss is zero: attention does not mix sequences


def test_a_g_loss_read_per_row_is_far_outside_the_parity_bound():
    """The defect case A of tests/test_gpu_train_grad_edges.py is there for: the backward reading one g_loss value per token row (or per
    sequence) instead of one per element.  Under the constant 1 / (B N 9) all of these are the same gradient; under TC.draw_g_loss
    every tensor that receives a gradient is beyond 4 x the float32 helper's own distance."""
    den = build_dropin(NONDEFAULT, seed=31)
    sd = {k: v.detach().clone() for k, v in den.state_dict().items()}
    net = TC.Net.of_cfg(NONDEFAULT)
    g = torch.Generator().manual_seed(5)
    B, N = 3, 7
    inp = {"x_start": torch.randn(B, N, 9, generator=g), "noise": torch.randn(B, N, 9, generator=g),
           "z": torch.randn(B, N, NONDEFAULT.z, generator=g), "t": torch.tensor([0, 99, 41])}
    g_loss = TC.draw_g_loss(B, N)
    r64 = TC.loss_and_grads(sd, net, inp, "pred_noise", "l1", g_loss=g_loss)
    forced = {"masks": r64["masks"], "signs": r64["signs"]}
    r32 = TC.loss_and_grads(sd, net, inp, "pred_noise", "l1", g_loss=g_loss, dtype=torch.float32, **forced)
    defects = {"per row": g_loss[:, :, 2:3].expand(B, N, 9), "per sequence": g_loss[:, 3:4, 4:5].expand(B, N, 9), "sign dropped": g_loss.abs()}
    for what, bad in defects.items():
        rbad = TC.loss_and_grads(sd, net, inp, "pred_noise", "l1", g_loss=bad, **forced)
        closest = min(TC.grad_dist(rbad["grads"][n], r64["grads"][n]) / TC.grad_dist(r32["grads"][n], r64["grads"][n]) for n in r64["grads"])
        print(f"g_loss {what}: the closest tensor is {closest:.1f} x own away")
        assert closest > 100.0, what


def _in_proj_like(d, q_share, own_rel, seed):
    """A synthetic [3 d, d] float64 'gradient' whose q rows are ``q_share`` of the v rows, and a float32-like copy ``own_rel`` away."""
    g = torch.Generator().manual_seed(seed)
    g64 = torch.randn(3 * d, d, generator=g, dtype=torch.float64)
    g64[:d] *= q_share
    own = g64 * (1.0 + own_rel * (2.0 * torch.rand(3 * d, d, generator=g, dtype=torch.float64) - 1.0))
    return g64, own


def test_block_rule_binds_a_q_block_the_tensor_rule_lets_through():
    """grad_blocks / block_misses: a 1e-3 relative error in the q rows of an in_proj gradient whose q rows are 0.5 % of the tensor's
    maximum (the v block) is 5e-6 of that maximum -- inside 4 x an own distance of 3e-6 -- and 1e-3 of the q block's own maximum."""
    d, name = 32, "_trunk.layers.0.self_attn.in_proj_weight"
    g64, own = _in_proj_like(d, q_share=0.005, own_rel=3e-6, seed=1)
    assert not TC.block_misses(name, own, own, g64, d, 5) and not TC.block_misses(name, g64, own, g64, d, 5)
    bad = own.clone()
    bad[:d] *= 1.001
    e, o = TC.grad_dist(bad, g64), TC.grad_dist(own, g64)
    assert e <= 4.0 * o, (e, o)                                        # the tensor rule passes
    misses = TC.block_misses(name, bad, own, g64, d, 5)
    assert [m[0] for m in misses] == [name + "[q]"] and misses[0][1] > 4.0 * misses[0][2]
    bad = own.clone()
    bad[d:2 * d] *= 1.001                                              # the k rows of the WEIGHT are bound, the k rows of the BIAS are not
    assert [m[0] for m in TC.block_misses(name, bad, own, g64, d, 5)] == [name + "[k]"]
    bname = "_trunk.layers.0.self_attn.in_proj_bias"
    assert not TC.block_misses(bname, bad[:, 0], own[:, 0], g64[:, 0], d, 5)
    zero = g64.clone()
    zero[:2 * d] = 0.0                                                 # N = 1: float64's q and k blocks are identically zero, so must g's be
    assert not TC.block_misses(name, zero.float(), zero.float(), zero, d, 5)
    tiny = zero.clone()
    tiny[0, 0] = 1e-30
    assert [m[0] for m in TC.block_misses(name, tiny, zero.float(), zero, d, 5)] == [name + "[q]"]
    # the recorded margin of one block reaches that block only
    assert not TC.block_misses(name, own * 1.0 + (own - g64) * 7.0, own, g64, d, 5, 4.0, {name + "[q]": 16.0, name + "[k]": 16.0, name + "[v]": 16.0})


def test_first_weight_blocks_are_the_denoisers_column_groups():
    for pivot in (0, 1):
        g = torch.arange(2 * (317 + 7 + pivot), dtype=torch.float64).reshape(2, -1)
        b = TC.grad_blocks("_first.weight", g, 2, 7)
        assert list(b) == ["harmonic", "x", "t_emb", "z"] + (["pivot"] if pivot else [])
        assert [v.shape[1] for v in b.values()] == [180, 9, 128, 7] + ([1] if pivot else [])
        assert torch.equal(torch.cat(list(b.values()), dim=1), g)
    assert TC.grad_blocks("_first.bias", torch.zeros(4), 2, 7) == {} and TC.grad_blocks("z", torch.zeros(3, 5, 7), 2, 7) == {}


def test_q_block_times_1_001_of_a_float32_helper_gradient_fails_the_block_rule():
    """On the helper's own float32 gradient (non-default configuration, (9, 15)): every in_proj tensor whose q block is scaled by 1.001
    fails the block rule.  Here the q rows are 9 % to 22 % of the tensor's maximum, so the tensor rule sees 1e-3 of them as well; the two
    rules part where the block is a smaller share of the tensor (the synthetic case above).  The figures are printed."""
    den = build_dropin(NONDEFAULT, seed=31)
    sd = {k: v.detach().clone() for k, v in den.state_dict().items()}
    net, d = TC.Net.of_cfg(NONDEFAULT), NONDEFAULT.d
    g = torch.Generator().manual_seed(6)
    inp = {"x_start": torch.randn(9, 15, 9, generator=g), "noise": torch.randn(9, 15, 9, generator=g),
           "z": torch.randn(9, 15, NONDEFAULT.z, generator=g), "t": torch.linspace(0, 99, 9).round().long()}
    r64 = TC.loss_and_grads(sd, net, inp, "pred_noise", "l1")
    r32 = TC.loss_and_grads(sd, net, inp, "pred_noise", "l1", masks=r64["masks"], signs=r64["signs"], dtype=torch.float32)
    for n in sd:
        if not n.endswith(("in_proj_weight", "in_proj_bias")):
            continue
        g64, own = r64["grads"][n], r32["grads"][n]
        assert not TC.block_misses(n, own, own, g64, d, NONDEFAULT.z)
        bad = own.clone()
        bad[:d] *= 1.001
        misses = TC.block_misses(n, bad, own, g64, d, NONDEFAULT.z)
        share = g64[:d].abs().max().item() / g64.abs().max().item()
        print(f"{n}: q share {share:.3f}; tensor rule {TC.grad_dist(bad, g64) / TC.grad_dist(own, g64):.1f} x own, "
              f"block rule {misses[0][1] / misses[0][2]:.1f} x own")
        assert [m[0] for m in misses] == [n + "[q]"]


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
