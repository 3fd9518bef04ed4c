"""Yardstick of the trainer's differentiable outputs (pd_train_backward_ex, pd_pose_to_camera_backward; include/pd_engine_train.h):
train_checks' teacher-forced float64 / float32 p_losses (ReLU masks and l1 signs forced as CONSTANTS; train_dropout_checks' four
dropout sites when asked for) extended with

  * x_0_pred by the schedule formulas of p_losses_cases.fp64_p_losses (gaussian_diffuser.py:190-194, :316): under pred_noise
    sqrt_recip[t] x_t - sqrt_recipm1[t] model_out, under pred_x0 model_out itself -- in the working dtype and differentiable;
  * the decoded cameras O.pose_encoding_to_camera(x_0_pred);
  * S = sum(g_loss loss) + sum(g_model_out model_out) + sum(g_x0_pred x_0_pred) + sum(w_R R) + sum(w_T T) + sum(w_f focal_length),
    every term optional (``None`` = absent), and its gradient with respect to every parameter and z by torch.autograd.grad.
Linear functionals of the outputs keep the float64 comparison clean: the only discontinuities of S are the forced ones and the clamp of
the focal length, whose branch the tests pin on float64 before the engine runs (``focal_edge_distance``).
Shared by tests/test_train_outputs_cpu.py, tests/test_gpu_train_outputs.py, tests/test_gpu_train_outputs_dropin.py and
tests/test_gpu_camera_decode_grad.py."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from oracle import pd_oracle as O
import train_checks as TC
import train_dropout_checks as TD

FOCAL = (1.8, 0.1, 20.0)                         # pose_encoding_to_camera's defaults: log_focal_length_bias, min, max


def draw_upstream(B: int, N: int, seed: int) -> torch.Tensor:
    """An upstream gradient [B, N, 9] in the style of train_checks.draw_g_loss that also serves (1, 1): randn / (B N 9), mixed signs,
    times a per-frame factor that spans three decades over the B N frames; no zeroed rows."""
    g = torch.Generator().manual_seed(8800 + 100 * B + N + seed)
    w = (10.0 ** torch.linspace(-3.0, 0.0, B * N))[torch.randperm(B * N, generator=g)].reshape(B, N, 1)
    return torch.randn(B, N, 9, generator=g) / (B * N * 9) * w


def draw_camera_weights(n: int, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Fixed weights of a linear functional on n decoded cameras: w_R [n, 3, 3], w_T [n, 3], w_f [n, 2], each of the order 1 / n."""
    g = torch.Generator().manual_seed(8900 + n + seed)
    return {"R": torch.randn(n, 3, 3, generator=g) / n, "T": torch.randn(n, 3, generator=g) / n, "focal_length": torch.randn(n, 2, generator=g) / n}


def x0_from(model_out: torch.Tensor, x_t: torch.Tensor, t: torch.Tensor, objective: str, tables: Dict[str, torch.Tensor]) -> torch.Tensor:
    """x_0_pred in the dtype of the arguments (fp64_p_losses' formulas, differentiable with respect to model_out)."""
    if objective != "pred_noise":
        return model_out
    at = lambda name: tables[name][t].reshape(-1, 1, 1)                         # noqa: E731
    return at("sqrt_recip_alphas_cumprod") * x_t - at("sqrt_recipm1_alphas_cumprod") * model_out


def camera_functional(cams: Dict[str, torch.Tensor], w: Dict[str, torch.Tensor]) -> torch.Tensor:
    """sum(w_R R) + sum(w_T T) + sum(w_f focal_length) over the keys ``w`` holds, in the cameras' dtype."""
    return sum((w[k].to(cams[k].dtype).reshape(cams[k].shape) * cams[k]).sum() for k in ("R", "T", "focal_length") if w.get(k) is not None)


def focal_edge_distance(x0: torch.Tensor, focal=FOCAL):
    """On a float64 x_0_pred [.., 9]: (share of the focal entries the clamp holds, smallest relative distance |f / edge - 1| of an
    unclamped f = exp(logFL + bias) to either clamp edge).  A distance far above fp32's rounding means both precisions take one branch."""
    bias, lo, hi = focal
    f = (x0.reshape(-1, 9)[:, 7:9].double() + bias).exp()
    dist = torch.minimum((f / lo - 1.0).abs(), (f / hi - 1.0).abs()).min().item()
    return ((f < lo) | (f > hi)).double().mean().item(), dist


def outputs_and_grads(sd: Dict[str, torch.Tensor], net: TC.Net, inp: Dict[str, torch.Tensor], objective: str, loss_type: str,
                      g_loss: Optional[torch.Tensor] = None, g_model_out: Optional[torch.Tensor] = None,
                      g_x0_pred: Optional[torch.Tensor] = None, cam_w: Optional[Dict[str, torch.Tensor]] = None, masks=None, signs=None,
                      dtype=torch.float64, want=None, drop=None, focal=FOCAL):
    """train_checks.loss_and_grads with the extra terms of S (module docstring); ``drop`` = (p, sites, seed, step) applies
    train_dropout_checks' dropout.  At least one term must be present.
    -> dict(loss, model_out, x_0_pred, x_t, cameras {R, T, focal_length}, grads {name: tensor, "z"}, pre, masks, signs)."""
    assert not (g_loss is None and g_model_out is None and g_x0_pred is None and cam_w is None), "S has no term"
    sd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    tables = O.diffusion_tables(dtype=dtype)
    x_start, noise, t = inp["x_start"].to(dtype), inp["noise"].to(dtype), inp["t"]
    z = inp["z"].detach().to(dtype).requires_grad_(True)
    x_t = TC.q_sample(x_start, noise, t, tables)
    if drop is not None and drop[0] > 0.0 and drop[1]:
        out, info = TD.denoiser_forward_dropout(sd, net, x_t, t, z, drop[1], (drop[0], drop[2], drop[3]), masks)
    else:
        out, info = TC.denoiser_forward(sd, net, x_t, t, z, masks)
    target = noise if objective == "pred_noise" else x_start
    d = out - target
    s = torch.sign(d.detach())
    if loss_type == "l1":
        s = s if signs is None else signs.to(dtype).reshape(d.shape)
        loss = d * s
    else:
        loss = d * d
    x0 = x0_from(out, x_t, t, objective, tables)
    cams = O.pose_encoding_to_camera(x0, *focal)
    S = 0.0
    for g, v in ((g_loss, loss), (g_model_out, out), (g_x0_pred, x0)):
        if g is not None:
            S = S + (g.to(dtype).reshape(v.shape) * v).sum()
    if cam_w is not None:
        S = S + camera_functional(cams, cam_w)
    names = list(sd) if want is None else [n for n in want if n != "z"]
    gs = torch.autograd.grad(S, [sd[n] for n in names] + [z], allow_unused=True)
    grads = {n: (torch.zeros_like(sd[n]) if v is None else v) for n, v in zip(names, gs[:-1])}
    grads["z"] = torch.zeros_like(z) if gs[-1] is None else gs[-1]
    return {"loss": loss.detach(), "model_out": out.detach(), "x_0_pred": x0.detach(), "x_t": x_t, "cameras": {k: v.detach() for k, v in cams.items()},
            "grads": grads, "pre": info["pre"], "masks": info["masks"], "signs": s}


def decode_grads(enc: torch.Tensor, g_R=None, g_T=None, g_f=None, dtype=torch.float64, focal=FOCAL) -> torch.Tensor:
    """d [sum(g_R R) + sum(g_T T) + sum(g_f focal_length)] / d enc [n, 9] by autograd of O.pose_encoding_to_camera in ``dtype``."""
    e = enc.detach().to(dtype).requires_grad_(True)
    S = camera_functional(O.pose_encoding_to_camera(e, *focal), {"R": g_R, "T": g_T, "focal_length": g_f})
    g, = torch.autograd.grad(S, [e])
    return g
