"""CPU: the step-relative group checks of tests/ggs_checks.py against the oracle itself.  The fp32 oracle passes them against fp64 (at the
bound rule's K = 1: it IS the yardstick); a copy of the fp64 result whose logFL or quaternion step is 10 % too large fails them.  The logFL
copy passes the whole-tensor `rel_err(out, ref) < 5e-5` the GPU tests asserted before, which is why the helper exists."""
import pytest
import torch

from conftest import rel_err
from ggs_checks import (FLOOR_GRAD, FLOOR_STEP, GROUPS, K_GRAD, K_STEP, bounds, grad_group_errs, oracle_loss_grad, oracle_optimize, step_group_errs,
                        within)
from oracle import pd_oracle as O
from posediffusion_amd import synth

CASES = {                    # frames, matches per pair, iter_num (x 2: all flags)
    "n12_x40_2_iterations": (12, 40, 2),
    "n33_x12_3_iterations": (33, 12, 3),
    "n64_x8_3_iterations": (64, 8, 3),
}


def _case(name):
    N, per_pair, iters = CASES[name]
    enc = synth.make_cameras(N, seed=700 + N)
    md = synth.make_matches(enc, 224, 224, per_pair=per_pair, seed=700 + N)
    pm = O.prepare_matches(md["kp1"], md["kp2"], md["i12"], md["img_shape"])
    return synth.perturb_pose(enc, seed=7 + N), pm, iters


def _scaled_step(x0, ref, group, factor):
    """x0 + the reference's step with `group`'s columns scaled by `factor`, stored in fp32 as an engine's result would be"""
    x0, ref = x0.double().reshape(-1, 9), ref.double().reshape(-1, 9)
    out = ref.clone()
    sl = GROUPS[group]
    out[:, sl] = x0[:, sl] + factor * (ref[:, sl] - x0[:, sl])
    return out.float().reshape(1, -1, 9)


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_group_check_passes_fp32_oracle_and_fails_a_10_percent_step(name):
    x0, pm, iters = _case(name)
    ref64, s64 = oracle_optimize(x0, pm, iter_num=iters)
    ref32, s32 = oracle_optimize(x0, pm, torch.float32, iter_num=iters)
    assert s64 == s32 == 2 * iters
    e32 = step_group_errs(ref32, x0, ref64)
    print(name, "fp32 oracle vs fp64, step-relative per group:", {g: f"{v:.1e}" for g, v in e32.items()})
    assert max(e32.values()) < FLOOR_STEP / 10, e32                     # the floor leaves room over the fp32 oracle's own rounding
    assert not within(e32, bounds(e32, 1.0, FLOOR_STEP))
    for group in ("logFL", "quaternion"):
        bad = _scaled_step(x0, ref64, group, 1.1)
        e = step_group_errs(bad, x0, ref64)
        assert within(e, bounds(e32, K_STEP, FLOOR_STEP)), (name, group, e)      # the step check sees the 10 % error ...
        assert abs(e[group] - 0.1) < 1e-2, e
        if group == "logFL":                                                      # ... the whole-tensor bound of the earlier tests does not
            assert rel_err(bad, ref32) < 5e-5, (name, group, rel_err(bad, ref32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_grad_group_check_sees_a_small_focal_gradient_error(name):
    """The logFL gradient is 1/20 .. 1/50 of the largest T / quaternion one: a 0.2 % error in it passes `rel_err(grad, go) < 1e-4` against
    the fp32 autograd, not the per-group check against fp64."""
    x0, pm, _ = _case(name)
    n64, _, g64 = oracle_loss_grad(x0, pm)
    n32, _, g32 = oracle_loss_grad(x0, pm, torch.float32)
    assert n64 == n32
    e32 = grad_group_errs(g32, g64)
    assert max(e32.values()) < FLOOR_GRAD / 10, e32
    bad = g32.clone()
    bad[..., GROUPS["logFL"]] *= 1.002
    assert within(grad_group_errs(bad, g64), bounds(e32, K_GRAD, FLOOR_GRAD))
    assert rel_err(bad, g32) < 1e-4
