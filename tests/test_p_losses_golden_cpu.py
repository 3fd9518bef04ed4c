"""CPU: tests/golden/p_losses.npz is consistent with itself -- its x_t, x_0_pred and losses follow from its inputs (redrawn from the
seeds), its timesteps and its own model output by the schedule formulas evaluated in float64 (gaussian_diffuser.py:211-216, :190-194,
:314-323).  Guards the generator (tools/make_p_losses_golden.py): a fixture recorded with the wrong t, objective or loss type fails here.

Bounds: every fixture value is an fp32 result of at most two products and one sum of fp32 operands, tables included (the reference
rounds its buffers to fp32, :157): |error| <= 8 x 2^-24 x (the sum of the magnitudes of the terms)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import pd_oracle as O
from p_losses_cases import CASES, LOSS_TYPES, OBJECTIVES, SEED, fp64_p_losses, inputs

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def gold():
    return load_golden("p_losses.npz")


def test_fixture_covers_the_cases(gold):
    assert int(gold["seed"]) == SEED
    for c in CASES:
        assert gold[f"{c.name}_t"].tolist() == list(c.t) and len(c.t) == c.B
        for obj in OBJECTIVES:
            for k in ("x_t", "x_0_pred", "model_out") + tuple(f"loss_{lt}" for lt in LOSS_TYPES):
                v = gold[f"{c.name}_{obj}_{k}"]
                assert v.shape == (c.B, c.N, 9) and v.dtype == np.float32 and np.isfinite(v).all(), (c.name, obj, k)
    ts = sorted({t for c in CASES for t in c.t})
    assert ts[0] == 0 and ts[-1] == 99                                         # both ends of the schedule


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c.name for c in CASES])
def test_fixture_follows_the_schedule_formulas(gold, ci, seeded_diffuser):
    from oracle.make_golden import weight_checksum
    np.testing.assert_allclose(weight_checksum(seeded_diffuser.model.state_dict()), gold["weight_checksum"], rtol=1e-9)
    c, inp = CASES[ci], inputs(ci)
    tb = O.diffusion_tables(dtype=torch.float64)
    at = lambda name: tb[name][inp["t"]].reshape(-1, 1, 1)                      # noqa: E731
    for obj in OBJECTIVES:
        get = lambda k: torch.from_numpy(gold[f"{c.name}_{obj}_{k}"])          # noqa: E731
        mo = get("model_out")
        want = fp64_p_losses(mo, inp["x_start"], inp["noise"], inp["t"], obj, tb)
        xs, nz = inp["x_start"].double(), inp["noise"].double()
        mag_xt = (at("sqrt_alphas_cumprod") * xs).abs() + (at("sqrt_one_minus_alphas_cumprod") * nz).abs()
        assert ((get("x_t").double() - want["x_t"]).abs() <= 8 * EPS * mag_xt + 1e-30).all(), (c.name, obj)
        assert torch.equal(get("x_t"), torch.from_numpy(gold[f"{c.name}_{OBJECTIVES[0]}_x_t"]))      # q_sample does not depend on the objective
        if obj == "pred_noise":
            # x_0_pred from the fixture's OWN fp32 x_t (the formula's input in the reference), then the same error model
            x0 = at("sqrt_recip_alphas_cumprod") * get("x_t").double() - at("sqrt_recipm1_alphas_cumprod") * mo.double()
            mag = (at("sqrt_recip_alphas_cumprod") * get("x_t").double()).abs() + (at("sqrt_recipm1_alphas_cumprod") * mo.double()).abs()
            assert ((get("x_0_pred").double() - x0).abs() <= 8 * EPS * mag + 1e-30).all(), (c.name, obj)
            target = nz
        else:
            assert torch.equal(get("x_0_pred"), mo)
            target = xs
        d = mo.double() - target
        assert ((get("loss_l1").double() - d.abs()) .abs() <= 2 * EPS * d.abs() + 1e-30).all(), (c.name, obj)
        assert ((get("loss_l2").double() - d * d).abs() <= 4 * EPS * d * d + 1e-30).all(), (c.name, obj)
        # the two objectives see the same network: the model output differs only through nothing at all
        assert torch.equal(mo, torch.from_numpy(gold[f"{c.name}_{OBJECTIVES[0]}_model_out"]))


def test_fixture_model_output_is_the_oracle_forward(gold, oracle_weights):
    """The recorded model output is the reference Denoiser at the per-sequence timesteps: the oracle's fp32 forward agrees to rounding
    (2e-5 per column group, the teacher-forced denoiser bound of the GPU suite) -- a fixture recorded with a shared t would not."""
    from conftest import pose_err
    for ci, c in enumerate(CASES[:3]):
        inp = inputs(ci)
        xt = torch.from_numpy(gold[f"{c.name}_pred_noise_x_t"])
        ref = O.denoiser_forward(oracle_weights, xt, inp["t"], inp["z"])
        assert pose_err(gold[f"{c.name}_pred_noise_model_out"], ref) < 2e-5, c.name
