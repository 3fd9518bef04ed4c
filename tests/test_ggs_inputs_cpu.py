"""CPU: the conditions tests/test_gpu_ggs_inputs.py rests on, asserted on the oracle alone (no GPU, no engine code).

  1. Regimes.  Per regime scene and setting (tests/ggs_input_cases.py), in the fp64 and the fp32 oracle alike: "clipped" settings have
     coef < 1 in every iteration of every stage, "unclipped" ones coef == 1; "crossing" has iterations on both sides in the all-groups stage;
     the unclamped clip ratio is more than 1 % away from 1 everywhere, and fp64 and fp32 agree on the branch of every iteration.
  2. Thresholds.  No match lies within the contract band (1e-4 relative) of sampson_max wherever the GPU tests compare valid counts: the
     start pose of every scene, and every iterate of the all-groups stage's trace in every setting.  ggs_checks.sampson_max_for then
     returns sampson_max itself.
  3. The checks see the errors they are for.  The fp64 oracle on mutated inputs -- h and w exchanged; learning_rate replaced by the
     default; the gradient doubled before the clip; momentum 0.9 where another value was asked for -- against the unmutated reference, with
     the checks and bounds the GPU tests use.  "Fails" means: some column group (or the gradient norm) exceeds 10 x its bound.  A doubled
     gradient and a wrong learning_rate PASS the step checks in the clipped settings -- that asymmetry is why the GPU tests leave the
     default setting -- while the in-loop gradient norm sees the doubled gradient there too.
"""
import pytest
import torch

import ggs_checks as G
import ggs_input_cases as Cs
from oracle import pd_oracle as O

REGIME_CASES = [(key, s) for key in Cs.REGIME_SCENES for s in Cs.settings_of(key)]
_id = lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def _coefs(trace):
    return [float(t["coef"]) for t in trace]


@pytest.mark.parametrize("key,setting", REGIME_CASES, ids=_id)
def test_regimes_hold_in_fp64_and_fp32(key, setting):
    regime = Cs.REGIME[setting]
    for fname in Cs.FLAGS:
        r = Cs.optimize_refs(key, setting, fname, Cs.REGIME_ITER_NUM[key[0]])
        c64, c32 = _coefs(r["trace64"]), _coefs(r["trace32"])
        want = Cs.REGIME_ITER_NUM[key[0]] * (2 if fname == "all" else 1)
        assert r["steps64"] == r["steps32"] == want == len(c64) == len(c32), (fname, r["steps64"], r["steps32"])
        # the UNCLAMPED ratio, not coef: 1.003 clamps to exactly 1, and the engine's fp32 ratio could then fall on the other side
        _, _, x0 = Cs.scene(*key)
        cfg = Cs.cfg_of(setting, key)
        q64, q32 = Cs.unclamped_ratios(r["trace64"], x0, cfg), Cs.unclamped_ratios(r["trace32"], x0, cfg)
        assert [min(q, 1.0) for q in q64] == pytest.approx(c64, rel=1e-12) and [min(q, 1.0) for q in q32] == pytest.approx(c32, rel=1e-5)
        assert not [q for q in q64 + q32 if abs(q - 1.0) <= 0.01], (fname, "a clip ratio within 1 % of 1", q64, q32)
        assert [c == 1.0 for c in c64] == [c == 1.0 for c in c32], (fname, "fp64 and fp32 take different branches", c64, c32)
        if regime == "clipped":
            assert max(c64 + c32) < 1.0, (fname, c64, c32)
        elif regime == "unclipped":
            assert min(c64 + c32) == 1.0, (fname, c64, c32)
        elif fname == "all":
            assert min(c64) < 1.0 and max(c64) == 1.0, (fname, c64)


def test_crossing_exists_where_the_module_says_so():
    assert set(Cs.CROSSING) == {(8, 224, 224), Cs.FIXTURE_SCENE, (33, 96, 512)}
    assert all(s in Cs.settings_of(Cs.FIXTURE_SCENE) for s in Cs.FIXTURE_SETTINGS)


@pytest.mark.parametrize("key", sorted(set(Cs.GEOMETRY_SCENES + Cs.REGIME_SCENES + Cs.MIXED_SCENES[:3])), ids=_id)
def test_no_match_near_the_threshold_at_the_start_pose(key):
    _, pm, x0 = Cs.scene(*key)
    assert Cs.threshold_margin(x0, pm) > Cs.BAND
    n64, _, _ = G.oracle_loss_grad(x0, pm)
    assert G.sampson_max_for(x0, pm, n64) == Cs.SAMPSON_MAX
    assert G.oracle_loss_grad(x0, pm, torch.float32)[0] == n64


@pytest.mark.parametrize("key,setting", REGIME_CASES, ids=_id)
def test_no_match_near_the_threshold_along_the_traced_iterates(key, setting):
    _, pm, _ = Cs.scene(*key)
    r = Cs.optimize_refs(key, setting, "all", Cs.REGIME_ITER_NUM[key[0]])
    for i, t in enumerate(r["trace64"][:-1]):                        # the last iterate is never evaluated
        assert Cs.threshold_margin(t["x"], pm) > Cs.BAND, (i, Cs.threshold_margin(t["x"], pm))
    assert [t["n_valid"] for t in r["trace64"]] == [t["n_valid"] for t in r["trace32"]]


# ------------------------------------------------------------------------------------------------ 3. mutations
def _optimize(x0, pm, flags, cfg, grad_scale=1.0):
    """GGS_optimize (geometry_guided_sampling.py:67-126) in fp64 with one hook: the gradient times `grad_scale` before the clip.  With
    grad_scale = 1 this is pd_oracle.ggs_optimize, which test_the_hooked_loop_is_the_oracle asserts."""
    x = G._x(x0, torch.float64).requires_grad_(True)
    alpha, lr, mom = cfg["alpha"], cfg["learning_rate"], cfg.get("momentum", 0.9)
    buf, trace = None, []
    with G.one_thread():
        for _ in range(cfg["iter_num"] * (2 if all(flags) else 1)):
            v, _ = O.compute_sampson_distance(x, pm, *flags, sampson_max=cfg["sampson_max"])
            loss = v.mean()
            (g,) = torch.autograd.grad(loss, x)
            g = g * grad_scale
            gnorm = g.norm()
            coef = torch.clamp(alpha * (x.detach() * (g.abs() > 0)).norm() / lr / (gnorm + 1e-6), max=1.0)
            g = g * coef
            buf = g.clone() if buf is None else mom * buf + g
            with torch.no_grad():
                x -= lr * buf
            trace.append({"x": x.detach().clone(), "loss": loss.detach(), "n_valid": len(v), "gnorm": gnorm.detach(), "coef": coef})
    return x.detach(), trace


def _mutants(key, setting):
    """{mutation: (pose, trace)} of the fp64 oracle on mutated inputs, all-groups stage"""
    _, pm, x0 = Cs.scene(*key)
    cfg = Cs.cfg_of(setting, key, iter_num=Cs.REGIME_ITER_NUM[key[0]])
    swapped = dict(pm, h=pm["w"], w=pm["h"])
    flags = Cs.FLAGS["all"]
    return {"hw_swapped": _optimize(x0, swapped, flags, cfg),
            "lr_default": _optimize(x0, pm, flags, dict(cfg, learning_rate=1e-2)),
            "grad_x2": _optimize(x0, pm, flags, cfg, grad_scale=2.0),
            "momentum_0.9": _optimize(x0, pm, flags, dict(cfg, momentum=0.9))}


def _excess(key, setting, x, trace):
    """(worst step error / its bound, worst gnorm error / its bound) of a result under check_steps and check_trace's rules"""
    _, _, x0 = Cs.scene(*key)
    r = Cs.optimize_refs(key, setting, "all", Cs.REGIME_ITER_NUM[key[0]])
    e, bnd = G.step_group_errs(x, x0, r["x64"]), G.bounds(G.step_group_errs(r["x32"], x0, r["x64"]), G.K_STEP, G.FLOOR_STEP)
    step = max(e[g] / bnd[g] for g in G.GROUPS)
    gn = 0.0
    for ei, bi, egn, bgn in G.trace_errs(G.trace_rows(trace), x0, r["trace64"], r["trace32"]):
        step = max(step, max(ei[g] / bi[g] for g in G.GROUPS))
        gn = max(gn, egn / bgn)
    return step, gn


@pytest.mark.parametrize("key,setting", REGIME_CASES, ids=_id)
def test_the_hooked_loop_is_the_oracle(key, setting):
    _, pm, x0 = Cs.scene(*key)
    r = Cs.optimize_refs(key, setting, "all", Cs.REGIME_ITER_NUM[key[0]])
    x, trace = _optimize(x0, pm, Cs.FLAGS["all"], Cs.cfg_of(setting, key, iter_num=Cs.REGIME_ITER_NUM[key[0]]))
    assert torch.equal(x, r["x64"]) and [float(t["gnorm"]) for t in trace] == [float(t["gnorm"]) for t in r["trace64"]]
    assert _excess(key, setting, x, trace) == (0.0, 0.0)


@pytest.mark.parametrize("key,setting", REGIME_CASES, ids=_id)
def test_checks_see_the_mutations_they_are_for(key, setting):
    regime = Cs.REGIME[setting]
    cfg = Cs.cfg_of(setting, key)
    res = {m: _excess(key, setting, *xt) for m, xt in _mutants(key, setting).items()}
    print(f"\n{key} {setting}: (step error, gnorm error) / bound:", {m: f"{s:.2g}, {g:.2g}" for m, (s, g) in res.items()})
    # exchanged h and w: grossly visible everywhere (the step, and the gradient norm) -- and an identity at a square image, which is
    # why the rest of the suite cannot see it
    if key[1] == key[2]:
        assert res["hw_swapped"] == (0.0, 0.0), res
    else:
        assert res["hw_swapped"][0] >= 10 and res["hw_swapped"][1] >= 10, res
    # the doubled gradient: the in-loop gradient norm sees it in every regime; the step only where an iteration is unclipped
    assert res["grad_x2"][1] >= 10, res
    if regime == "clipped":
        assert res["grad_x2"][0] <= 1 and res["lr_default"][0] <= 1 and res["lr_default"][1] <= 1, res
    else:
        assert res["grad_x2"][0] >= 10 and res["lr_default"][0] >= 10, res
    # momentum: an identity where 0.9 was asked for
    if cfg.get("momentum", 0.9) == 0.9:
        assert res["momentum_0.9"] == (0.0, 0.0), res
    else:
        assert res["momentum_0.9"][0] >= 10, res


@pytest.mark.parametrize("key", Cs.GEOMETRY_SCENES, ids=_id)
def test_exchanged_height_and_width_fail_the_gradient_check(key):
    """check_loss_grad's rule on the fp64 oracle with h and w exchanged: another valid count, and a gradient off by >= 10 x the bound"""
    _, pm, x0 = Cs.scene(*key)
    n64, _, g64 = G.oracle_loss_grad(x0, pm)
    _, _, g32 = G.oracle_loss_grad(x0, pm, torch.float32)
    ns, _, gs = G.oracle_loss_grad(x0, dict(pm, h=pm["w"], w=pm["h"]))
    e, bnd = G.grad_group_errs(gs, g64), G.bounds(G.grad_group_errs(g32, g64), G.K_GRAD, G.FLOOR_GRAD)
    assert ns != n64 and max(e[g] / bnd[g] for g in G.GROUPS) >= 10, (n64, ns, e, bnd)
