"""No GPU: the C-ABI of the trainer's differentiable outputs (pd_train_backward_ex, pd_pose_to_camera_backward in
include/pd_engine_train.h; tests/test_train_abi_cpu.py holds header and binding together), the host-side rules of the opt-in, and the
yardstick tests/train_outputs_checks.py against plain autograd of the oracle."""
import inspect

import pytest
import torch

from oracle import pd_oracle as O
from p_losses_cases import fp64_p_losses, inputs
import train_checks as TC
import train_outputs_checks as TO
from posediffusion_amd import _lib, synth
from posediffusion_amd.train import PoseTrainer, p_losses_with_grad


@pytest.fixture(scope="module")
def sd64(oracle_weights):
    return O.cast_state_dict(oracle_weights, torch.float64)


def test_new_symbols_are_exported_and_refuse_null_handles_and_absent_upstreams_by_name():
    lib = _lib.load()
    for name in ("pd_train_backward_ex", "pd_pose_to_camera_backward"):
        assert name in _lib.TRAIN_SIGNATURES and getattr(lib, name).argtypes == _lib.TRAIN_SIGNATURES[name][1]
    assert lib.pd_train_backward_ex(None, None, None, None, None, None, None, None) == -1
    assert "pd_train_backward_ex" in _lib.last_error()
    assert lib.pd_pose_to_camera_backward(None, None, None, None, 1, 1.8, 0.1, 20.0, None, None) == -1
    assert "pd_pose_to_camera_backward" in _lib.last_error()
    # valid-looking pointers, no upstream: refused before anything is read or launched (host memory is never dereferenced on the host)
    buf = (_lib.C.c_float * 9)()
    addr = _lib.C.addressof(buf)
    assert lib.pd_pose_to_camera_backward(addr, None, None, None, 1, 1.8, 0.1, 20.0, addr, None) == -1
    assert "pd_pose_to_camera_backward" in _lib.last_error() and "all NULL" in _lib.last_error()
    assert lib.pd_pose_to_camera_backward(addr, addr, None, None, 0, 1.8, 0.1, 20.0, addr, None) == -1
    assert "n_cameras=0" in _lib.last_error()


def test_opt_ins_default_off_and_signatures():
    diff = synth.make_diffuser(seed=0, num_layers=1)
    assert diff.engine_grad is False and diff.engine_grad_outputs is False
    assert inspect.signature(p_losses_with_grad).parameters["differentiable_outputs"].default is False
    assert list(inspect.signature(PoseTrainer.backward).parameters) == ["self", "params", "g_loss", "want", "g_model_out", "g_x0_pred"]
    assert all(inspect.signature(PoseTrainer.backward).parameters[k].default is None for k in ("g_loss", "want", "g_model_out", "g_x0_pred"))


def test_x0_is_fp64_p_losses_formula(sd64):
    inp = inputs(1)
    tb = O.diffusion_tables(dtype=torch.float64)
    for objective in ("pred_noise", "pred_x0"):
        r = TO.outputs_and_grads(sd64, TC.DEFAULT_NET, inp, objective, "l1", g_x0_pred=TO.draw_upstream(3, 5, 1), want=[])
        ref = fp64_p_losses(r["model_out"], inp["x_start"], inp["noise"], inp["t"], objective, tb)
        assert torch.equal(r["x_0_pred"], ref["x_0_pred"]) and torch.equal(r["x_t"], ref["x_t"]) and torch.equal(r["loss"], ref["loss_l1"])
        cams = O.pose_encoding_to_camera(ref["x_0_pred"])
        assert all(torch.equal(r["cameras"][k], cams[k]) for k in cams)


@pytest.mark.parametrize("objective,loss_type", [("pred_noise", "l1"), ("pred_x0", "l2")])
def test_autograd_with_own_masks_is_plain_autograd_of_the_unforced_network(sd64, objective, loss_type):
    """All terms of S at once, the helper with its OWN masks against torch.abs / torch.relu autograd of O.denoiser_forward: forcing a
    function's own masks changes nothing where no mask flips (one dtype, one run: none can)."""
    inp = inputs(1)
    B, N, _ = inp["x_start"].shape
    ups = [TO.draw_upstream(B, N, s) for s in (1, 2, 3)]
    cam_w = TO.draw_camera_weights(B * N)
    mine = TO.outputs_and_grads(sd64, TC.DEFAULT_NET, inp, objective, loss_type, *ups, cam_w=cam_w)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in sd64.items()}
    z = inp["z"].double().requires_grad_(True)
    tb = O.diffusion_tables(dtype=torch.float64)
    x_start, noise, t = inp["x_start"].double(), inp["noise"].double(), inp["t"]
    x_t = TC.q_sample(x_start, noise, t, tb)
    out = O.denoiser_forward(sd, x_t, t, z)
    d = out - (noise if objective == "pred_noise" else x_start)
    loss = d.abs() if loss_type == "l1" else d * d
    c, cm1 = (tb[k][t].reshape(-1, 1, 1) for k in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod"))
    x0 = c * x_t - cm1 * out if objective == "pred_noise" else out
    cams = O.pose_encoding_to_camera(x0)
    S = sum((g.double() * v).sum() for g, v in zip(ups, (loss, out, x0))) + sum((cam_w[k].double() * cams[k]).sum() for k in cams)
    names = list(sd)
    gs = torch.autograd.grad(S, [sd[n] for n in names] + [z])
    for n, g in zip(names + ["z"], gs):
        assert TC.grad_dist(mine["grads"][n], g) <= 1e-12, n
    # each extra term moves the gradient: none is silently dropped by the helper
    base = TO.outputs_and_grads(sd64, TC.DEFAULT_NET, inp, objective, loss_type, ups[0], want=["_last.3.weight"])["grads"]["_last.3.weight"]
    for kw in ({"g_model_out": ups[1]}, {"g_x0_pred": ups[2]}, {"cam_w": cam_w}):
        more = TO.outputs_and_grads(sd64, TC.DEFAULT_NET, inp, objective, loss_type, ups[0], want=["_last.3.weight"], **kw)["grads"]["_last.3.weight"]
        assert TC.grad_dist(more, base) > 1e-3, kw.keys()


def test_decode_grads_columns():
    """The decode's gradient by column group on float64: T is copied, the quaternion columns are orthogonal to q (R does not depend on
    |q|: two_s = 2 / |q|^2 normalises), clamped focal entries get exactly 0 and the others g_f * f."""
    g = torch.Generator().manual_seed(5)
    n = 12
    enc = torch.randn(n, 9, generator=g, dtype=torch.float64)
    enc[:, 7:9] = torch.tensor([-5.0, 0.0, 2.0], dtype=torch.float64)[torch.arange(2 * n) % 3].reshape(n, 2)      # f = 0.04 / 6.0 / 44.7
    w = TO.draw_camera_weights(n)
    ge = TO.decode_grads(enc, w["R"], w["T"], w["focal_length"])
    assert torch.equal(ge[:, :3], w["T"].double())
    assert ((ge[:, 3:7] * enc[:, 3:7]).sum(-1).abs() <= 1e-12 * ge[:, 3:7].abs().max()).all()
    f = (enc[:, 7:9] + 1.8).exp()
    inside = (f >= 0.1) & (f <= 20.0)
    assert inside.any() and (~inside).any() and (ge[:, 7:9][~inside] == 0).all()
    assert torch.allclose(ge[:, 7:9][inside], (w["focal_length"].double() * f)[inside], rtol=1e-14, atol=0)
    share, dist = TO.focal_edge_distance(enc)
    assert abs(share - 2 / 3) < 1e-12 and dist > 0.5
