"""Step-relative, per-column-group checks of GGS results against the fp64 oracle (a plain helper module, imported by the tests).

A few GGS_optimize iterations move a pose by 1e-4 .. 1e-2 while |T| ~ 6 and |logFL| ~ 0.8: a whole-tensor (or per-group) relative error of
the OUTPUT mostly compares the unchanged input with itself -- a focal update 10 % too large passes `rel_err(out, ref) < 5e-5`.  These helpers
compare the STEP (out - x0) with the oracle's step, per column group (T / quaternion / logFL), each scaled by the oracle's largest step in
that group; gradients per group, each scaled by its own largest magnitude.

The reference is the oracle in fp64 (one CPU thread: its sums do not depend on the host).  The bound rule, per group:
    err <= max(K x (the fp32 oracle's own distance from fp64), floor)
-- the rule of test_sampson_loss_and_gradient_vs_reference_fixture, with a floor far under 0.1 so that a 10 % error in any group's step fails.
"""
import contextlib

import torch

from oracle import pd_oracle as O

GROUPS = {"T": slice(0, 3), "quaternion": slice(3, 7), "logFL": slice(7, 9)}
# Measured on gfx950 over every kernel family and frame count in the suite: the engine's step is 1e-5 .. 3e-3 of the oracle's step from fp64
# (mostly the fp32 storage of x, which the fp32 oracle shares: 1e-5 .. 6e-3), its gradient 2e-6 .. 3e-5 of each group's scale
K_STEP, FLOOR_STEP = 4.0, 1e-2          # step of GGS_optimize / ggs_guide against fp64
K_GRAD, FLOOR_GRAD = 4.0, 1e-4          # analytic gradient against fp64's autograd


@contextlib.contextmanager
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _rows(a):
    return torch.as_tensor(a).detach().cpu().double().reshape(-1, 9)


def step_group_errs(out, x0, ref):
    """{group: max|(out - x0) - (ref - x0)| / max|ref - x0|} over that group's columns (poses [.., 9] or [.., N*9])."""
    out, x0, ref = _rows(out), _rows(x0), _rows(ref)
    d, s = out - ref, ref - x0
    return {g: (d[:, sl].abs().max() / s[:, sl].abs().max().clamp_min(1e-30)).item() for g, sl in GROUPS.items()}


def grad_group_errs(grad, ref_grad):
    """{group: max|grad - ref| / max|ref|} over that group's columns."""
    a, b = _rows(grad), _rows(ref_grad)
    return {g: ((a[:, sl] - b[:, sl]).abs().max() / b[:, sl].abs().max().clamp_min(1e-30)).item() for g, sl in GROUPS.items()}


def bounds(e32, k, floor):
    """{group: max(k x e32[group], floor)}"""
    return {g: max(k * e32[g], floor) for g in GROUPS}


def within(errs, bnd):
    """The groups whose error exceeds its bound ({} when every group passes)."""
    return {g: (errs[g], bnd[g]) for g in GROUPS if not errs[g] <= bnd[g]}


def _x(x0, dtype):
    return torch.as_tensor(x0).detach().cpu().to(dtype).reshape(1, -1, 9).clone()


def oracle_loss_grad(x0, pm, dtype=torch.float64, sampson_max=10.0, flags=(True, True, True)):
    """(valid count, mean Sampson distance, gradient) of compute_sampson_distance + autograd in `dtype`."""
    with one_thread():
        x = _x(x0, dtype).requires_grad_(True)
        v, _ = O.compute_sampson_distance(x, pm, *flags, sampson_max=sampson_max)
        (g,) = torch.autograd.grad(v.mean(), x)
    return len(v), v.mean().item(), g


def sampson_max_for(x0, pm, n_valid, sampson_max=10.0, band=1e-4):
    """The threshold at which fp64 admits exactly the `n_valid` smallest Sampson values: `sampson_max` itself when that is fp64's own
    count, else the midpoint between the two values around the cut -- asserted to lie within `band` (relative) of sampson_max, the contract
    band in which the engine's fp32 Sampson value may fall on the other side of the threshold."""
    with one_thread():
        s, _ = O.compute_sampson_distance(_x(x0, torch.float64), pm, sampson_max=float("inf"))
    s = torch.sort(s.detach()).values
    if int((s < sampson_max).sum()) == n_valid:
        return sampson_max
    assert 0 < n_valid < len(s), n_valid
    smax = float(0.5 * (s[n_valid - 1] + s[n_valid]))
    assert abs(smax - sampson_max) <= band * sampson_max, ("valid count outside the contract band of sampson_max", n_valid, smax)
    return smax


def oracle_optimize(x0, pm, dtype=torch.float64, **cfg):
    """(pose, iterations stepped) of GGS_optimize in `dtype`."""
    with one_thread():
        x, _, steps = O.ggs_optimize(_x(x0, dtype), pm, **cfg)
    return x, steps


def oracle_guide(x0, md, cfg, dtype=torch.float64):
    """(pose, iterations per stage) of geometry_guided_sampling's five stages in `dtype`."""
    steps = []
    with one_thread():
        x = O.geometry_guided_sampling(_x(x0, dtype), 0, md, cfg, steps=steps)
    return x, steps


def check_loss_grad(loss, grad, x0, pm, tag="", cache=None):
    """Engine (loss row [mean, valid count, ..], gradient [1, N, 9]) of ONE sequence against fp64: the valid count equal to fp64's (the
    threshold-adjusted oracle where a match lies within the contract band of sampson_max), the mean within 2e-5, the gradient per group
    within max(K_GRAD x fp32 oracle's distance, FLOOR_GRAD).  `cache` (a dict) keeps the oracle's results per valid count across calls
    with the same x0 and matches.  Returns the per-group errors and bounds."""
    n = int(loss[1])
    cache = {} if cache is None else cache
    if n not in cache:
        smax = sampson_max_for(x0, pm, n)
        n64, m64, g64 = oracle_loss_grad(x0, pm, sampson_max=smax)
        assert n == n64, (tag, n, n64)
        _, _, g32 = oracle_loss_grad(x0, pm, torch.float32, sampson_max=smax)
        cache[n] = (m64, g64, bounds(grad_group_errs(g32, g64), K_GRAD, FLOOR_GRAD))
    m64, g64, bnd = cache[n]
    assert abs(float(loss[0]) - m64) < 2e-5 * m64, (tag, float(loss[0]), m64)
    e = grad_group_errs(grad, g64)
    assert not within(e, bnd), (tag, "gradient per group vs fp64", within(e, bnd))
    return e, bnd


def check_steps(out, x0, ref64, ref32, tag=""):
    """Engine pose after some iterations against fp64, step-relative per group; `ref32` is the fp32 oracle's pose (the bound's yardstick)."""
    e, bnd = step_group_errs(out, x0, ref64), bounds(step_group_errs(ref32, x0, ref64), K_STEP, FLOOR_STEP)
    assert not within(e, bnd), (tag, "step per group vs fp64", within(e, bnd))
    return e, bnd


def trace_rows(trace):
    """An oracle trace (pd_oracle.ggs_optimize(trace=[..])) as rows (pose after the iteration, loss, valid count, |g| before the clip)."""
    return [(t["x"], float(t["loss"]), int(t["n_valid"]), float(t["gnorm"])) for t in trace]


def engine_trace_rows(tr, n_frames, iters):
    """The engine's trace of ONE sequence (ggs_optimize(trace=True)[2][b]: [iters, N*9 + 3]) as the same rows."""
    tr = torch.as_tensor(tr).detach().cpu()
    w = n_frames * 9
    return [(tr[i, :w], float(tr[i, w]), int(tr[i, w + 1]), float(tr[i, w + 2])) for i in range(iters)]


def trace_errs(rows, x0, trace64, trace32):
    """Rows of a per-iteration trace against the fp64 oracle's, iteration by iteration: the pose per column group relative to the ORACLE'S
    step of that iteration (step_group_errs from the oracle's previous iterate), and |g| before the clip relative to the oracle's; each
    with the bound its rule gives from the fp32 oracle's own distance (K_STEP / FLOOR_STEP, K_GRAD / FLOOR_GRAD).
    Returns [(step errors, step bounds, gnorm error, gnorm bound)] per iteration."""
    out = []
    prev = _x(x0, torch.float64)
    for (x, _, _, gn), t64, t32 in zip(rows, trace64, trace32):
        e = step_group_errs(x, prev, t64["x"])
        bnd = bounds(step_group_errs(t32["x"], prev, t64["x"]), K_STEP, FLOOR_STEP)
        g64 = float(t64["gnorm"])
        out.append((e, bnd, abs(gn - g64) / g64, max(K_GRAD * abs(float(t32["gnorm"]) - g64) / g64, FLOOR_GRAD)))
        prev = t64["x"]
    return out


def check_trace(rows, x0, trace64, trace32, tag=""):
    """Every iteration of a trace against fp64: pose per group (rule of check_steps, per iteration), valid count equal, loss within 1e-4
    relative (the bound of test_ggs_per_iteration_trace_vs_oracle), |g| before the clip under the gradient rule.  Returns the worst
    (step errors per group, gnorm error, gnorm bound at that iteration)."""
    assert len(rows) == len(trace64) == len(trace32), (tag, len(rows), len(trace64), len(trace32))
    worst, worst_gn = {g: 0.0 for g in GROUPS}, (0.0, FLOOR_GRAD)
    for i, ((_, loss, n, _), t64, (e, bnd, egn, bgn)) in enumerate(zip(rows, trace64, trace_errs(rows, x0, trace64, trace32))):
        assert n == t64["n_valid"], (tag, i, "valid count", n, t64["n_valid"])
        assert abs(loss - float(t64["loss"])) < 1e-4 * abs(float(t64["loss"])), (tag, i, "loss", loss, float(t64["loss"]))
        assert not within(e, bnd), (tag, i, "step of this iteration per group vs fp64", within(e, bnd))
        assert egn <= bgn, (tag, i, "|g| before the clip vs fp64", egn, bgn)
        worst = {g: max(worst[g], e[g]) for g in GROUPS}
        worst_gn = max(worst_gn, (egn, bgn))
    return worst, worst_gn[0], worst_gn[1]
