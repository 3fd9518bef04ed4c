"""GPU (-m gpu): the optimiser step on the engine (posediffusion_amd/optim.py, include/pd_engine_optim.h) -- the global gradient
norm, the clip coefficient and AdamW -- against the fp64 yardstick and the per-element bounds of tests/optim_checks.py, the exact equalities
between engine runs (repeat, 4-byte against 16-byte load path, handle capacity, with and without synchronisation), PyTorch's own pairing
over ten steps, state interchange with torch.optim.AdamW, and one training step end to end through the drop-in."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import optim_checks as OC
from posediffusion_amd import _lib, optim, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = OC.sizes(optim.CHUNK)


def _dev(a, views=False):
    """a fresh device tensor of the fp32 array `a`, or (views) a view at an odd element offset into a larger buffer: 4 bytes off 16"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    if not views:
        return t
    buf = torch.zeros(t.numel() + 5, device=DEV)
    v = buf[1:1 + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _build(case, views=False, spare=0, cls=optim.EngineAdamW, **kw):
    """(optimizer, parameters in the case's order) with gradients set and the case's state loaded; spare: that many more elements in a
    parameter without a gradient (a handle of larger capacity)"""
    params = [torch.nn.Parameter(_dev(p, views)) for p in case["p"]]
    for p, g in zip(params, case["g"]):
        p.grad = _dev(g, views)
    groups = [dict(h, params=[p for p, gi in zip(params, case["group"]) if gi == j]) for j, h in enumerate(case["groups"])]
    if spare:
        groups[0]["params"] = groups[0]["params"] + [torch.nn.Parameter(torch.zeros(spare, device=DEV)), torch.nn.Parameter(torch.zeros(3, device=DEV))]
    opt = cls(groups, **kw)
    if views:            # a loaded state would be fresh allocations: put the views in place
        for i, p in enumerate(params):
            if case["step"][i] > 1:
                opt.state[p] = dict(step=torch.tensor(float(case["step"][i] - 1)), exp_avg=_dev(case["m"][i], True), exp_avg_sq=_dev(case["v"][i], True))
    else:
        order = [p for g in opt.param_groups for p in g["params"]]
        state = {}
        for i, p in enumerate(params):
            if case["step"][i] > 1:
                state[next(k for k, q in enumerate(order) if q is p)] = dict(step=torch.tensor(float(case["step"][i] - 1)),
                                                                            exp_avg=torch.from_numpy(case["m"][i]), exp_avg_sq=torch.from_numpy(case["v"][i]))
        sd = opt.state_dict()
        sd["state"] = state
        opt.load_state_dict(sd)
    return opt, params


def _results(opt, params):
    st = [opt.state[p] for p in params]
    return ([p.detach().cpu().numpy() for p in params], [s["exp_avg"].cpu().numpy() for s in st], [s["exp_avg_sq"].cpu().numpy() for s in st])


def _run(case, **kw):
    """one engine step of `case`: (p, m, v, norm) on the host"""
    opt, params = _build(case, **kw)
    opt.step(max_grad_norm=case["max_norm"])
    for i, p in enumerate(params):
        assert float(opt.state[p]["step"]) == case["step"][i] and opt.state[p]["step"].device.type == "cpu"
        assert _same_bits([p.grad.cpu().numpy()], [case["g"][i]])                        # the step leaves the gradients as they were
    return _results(opt, params) + (opt.grad_norm.item(),)


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _assert_within(case, p, m, v, norm=None):
    w = OC.check_case(case, p, m, v, norm)
    print(f"{case['name']}: worst error / bound {', '.join(f'{k} {x:.3f}' for k, x in w.items())}")
    assert all(x <= 1.0 for x in w.values()), w


def _with_grads(arrays):
    ps = []
    for g in arrays:
        p = torch.nn.Parameter(torch.zeros(len(g), device=DEV))
        p.grad = _dev(g)
        ps.append(p)
    return ps


# ---- 1. the norm ------------------------------------------------------------------------------------
def test_norm_over_the_size_list_and_over_300_small_tensors():
    for name, size_list in (("size list", SIZES), ("300 x 7", [7] * 300)):
        g = OC.norm_values(size_list, seed=len(size_list))
        n64 = OC.norm64(g)
        got = optim.grad_norm(_with_grads(g)).item()
        print(f"{name}: norm {got:.9e}, fp64 {n64:.9e}, error / bound {abs(got - n64) / OC.norm_bound(n64):.3f}")
        assert np.isfinite(n64) and n64 > 1e17 and abs(got - n64) <= OC.norm_bound(n64)
        small = [x for x in g if len(x) <= 257]                                          # a sum the largest values do not swamp
        small = [np.where(np.abs(x) > 1.0, np.float32(1e-3), x) for x in small]
        n64 = OC.norm64(small)
        assert abs(optim.grad_norm(_with_grads(small)).item() - n64) <= OC.norm_bound(n64)


def test_norm_propagates_nan_and_inf_and_is_zero_for_nothing():
    g = OC.norm_values(SIZES, seed=5)
    g[8][-1] = np.inf
    assert optim.grad_norm(_with_grads(g)).item() == np.inf
    g[3][17] = np.nan
    assert np.isnan(optim.grad_norm(_with_grads(g)).item())
    assert optim.grad_norm(_with_grads([np.zeros(5, np.float32)])).item() == 0.0
    assert optim.grad_norm([torch.nn.Parameter(torch.zeros(3, device=DEV))]).item() == 0.0     # no gradient at all


# ---- 2. one step against fp64 -----------------------------------------------------------------------
@pytest.mark.parametrize("case", OC.step_cases(), ids=lambda c: c["name"])
def test_one_step_against_fp64(case):
    p, m, v, norm = _run(case)
    _assert_within(case, p, m, v, norm)                                                 # (the norm is computed without clipping too)


# ---- 3. clipping ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OC.clip_cases(), ids=lambda c: c["name"])
def test_clipped_step_against_fp64(case):
    p, m, v, norm = _run(case)
    _assert_within(case, p, m, v, norm)
    if OC.norm64(case["g"]) < 0.5 * case["max_norm"]:                                   # the coefficient is exactly 1: the bits of an unclipped step
        off = _run(dict(case, max_norm=None))
        assert off[3] == norm and _same_bits(p + m + v, off[0] + off[1] + off[2])
    else:
        off = _run(dict(case, max_norm=None))
        assert not _same_bits(m, off[1])


def test_a_nan_gradient_makes_every_updated_parameter_nan_as_in_pytorch():
    case = OC.make_case("nan", gscale=10.0, max_norm=1.0, seed=40)
    case["g"][4][11] = np.nan
    p, m, v, norm = _run(case)
    ref, rparams = _build(case, cls=torch.optim.AdamW)
    torch.nn.utils.clip_grad_norm_(rparams, 1.0)
    ref.step()
    assert np.isnan(norm) and all(np.isnan(x).all() for x in p) and all(bool(torch.isnan(q).all()) for q in rparams)
    case = OC.make_case("inf", gscale=10.0, max_norm=1.0, seed=41)                       # an inf norm: coefficient 0, inf * 0 = NaN in that element alone
    case["g"][4][11] = np.inf
    p, m, v, norm = _run(case)
    ref, rparams = _build(case, cls=torch.optim.AdamW)
    torch.nn.utils.clip_grad_norm_(rparams, 1.0)
    ref.step()
    assert norm == np.inf
    for x, q in zip(p, rparams):
        assert np.array_equal(np.isnan(x), torch.isnan(q).cpu().numpy())
    assert np.isnan(p[4][11]) and sum(int(np.isnan(x).sum()) for x in p) == 1


def test_clip_grad_norm_alone_against_pytorch():
    for gscale in (1e-3, 30.0):
        case = OC.make_case("clip_alone", gscale=gscale, seed=42)
        ours, theirs = _with_grads(case["g"]), _with_grads(case["g"])
        norm = optim.clip_grad_norm_(ours, 1.0)
        ref = torch.nn.utils.clip_grad_norm_(theirs, 1.0)
        n64 = OC.norm64(case["g"])
        assert norm.shape == () and norm.dtype == torch.float32 and norm.device.type == "cuda"
        assert abs(norm.item() - n64) <= OC.norm_bound(n64)
        worst = 0.0
        for a, b in zip(ours, theirs):
            a, b = a.grad.cpu().numpy(), b.grad.cpu().numpy()
            worst = max(worst, float(np.max(np.abs(a.astype(np.float64) - b) / np.spacing(np.abs(b)))))
        print(f"gradient scale {gscale:g}: norm {norm.item():.7e} (PyTorch {ref.item():.7e}), scaled gradients at most {worst:.2f} ulp from PyTorch's")
        assert worst <= 2.0
        if gscale < 1.0:
            assert _same_bits([a.grad.cpu().numpy() for a in ours], case["g"])           # below max_norm nothing changes


# ---- 4. exact equalities between engine runs ----------------------------------------------------------
EXACT = OC.make_case("exact", steps=[1, 1000, 3], gscale=5.0, max_norm=1.0, groups=[OC.hp(), OC.hp(lr=1e-2, betas=(0.5, 0.9))], group=[0, 1], seed=50)


@pytest.fixture(scope="module")
def exact_run():
    return _run(EXACT)


def test_the_same_step_twice_gives_the_same_bits(exact_run):
    again = _run(EXACT)
    _assert_within(EXACT, *exact_run)
    assert again[3] == exact_run[3] and _same_bits(sum(again[:3], []), sum(exact_run[:3], []))


def test_views_at_an_odd_offset_give_the_bits_of_fresh_allocations(exact_run):
    views = _run(EXACT, views=True)
    assert views[3] == exact_run[3] and _same_bits(sum(views[:3], []), sum(exact_run[:3], []))


def test_a_handle_of_larger_capacity_gives_the_same_bits(exact_run):
    big = _run(EXACT, spare=3 * optim.CHUNK + 1)
    assert big[3] == exact_run[3] and _same_bits(sum(big[:3], []), sum(exact_run[:3], []))
    params = _with_grads(EXACT["g"])
    a, b = optim.grad_norm(params), optim.grad_norm(params, capacity=(len(params), sum(len(g) for g in EXACT["g"])))
    assert a.item() == b.item() == exact_run[3]


# ---- 5. no hidden synchronisation dependence ----------------------------------------------------------
def test_three_steps_back_to_back_equal_three_synchronised_steps():
    rng = np.random.default_rng(60)
    grads = [[(3.0 * rng.standard_normal(s)).astype(np.float32) for s in SIZES] for _ in range(3)]
    case = OC.make_case("b2b", seed=61)
    out = []
    for sync in (False, True):
        opt, params = _build(case, max_grad_norm=1.0)
        host = [[torch.from_numpy(g).pin_memory() for g in step] for step in grads]
        norms = []
        for step in host:
            for p, g in zip(params, step):
                p.grad = None                                                            # the previous gradient tensors are dropped ...
            for p, g in zip(params, step):
                p.grad = g.to(DEV, non_blocking=True)                                    # ... and fresh ones allocated, no synchronisation
            opt.step()
            norms.append(opt.grad_norm)
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        out.append((_results(opt, params), [n.item() for n in norms]))
    assert out[0][1] == out[1][1] and len(set(out[0][1])) == 3
    assert _same_bits(sum(out[0][0], []), sum(out[1][0], []))


# ---- 6. against PyTorch over several steps ------------------------------------------------------------
def test_ten_steps_against_pytorch_and_fp64():
    rng = np.random.default_rng(70)
    steps = 10
    grads = [[(rng.standard_normal(s) * 10.0 ** rng.uniform(-2, 1)).astype(np.float32) for s in SIZES] for _ in range(steps)]
    case = OC.make_case("parity", seed=71)
    h = case["groups"][0]
    eng, eparams = _build(case, max_grad_norm=1.0)
    ref, rparams = _build(case, cls=torch.optim.AdamW)
    p64 = [p.astype(np.float64) for p in case["p"]]
    m64, v64 = [np.zeros_like(p) for p in p64], [np.zeros_like(p) for p in p64]
    for k in range(steps):
        for p, q, g in zip(eparams, rparams, grads[k]):
            p.grad, q.grad = _dev(g), _dev(g)
        eng.step()
        torch.nn.utils.clip_grad_norm_(rparams, 1.0)
        ref.step()
        coef = OC.coef64(OC.norm64(grads[k]), 1.0)
        for i in range(len(p64)):
            g = grads[k][i].astype(np.float64) * coef
            m64[i] = h["betas"][0] * m64[i] + (1 - h["betas"][0]) * g
            v64[i] = h["betas"][1] * v64[i] + (1 - h["betas"][1]) * g * g
            denom = np.sqrt(v64[i]) / np.sqrt(1 - h["betas"][1] ** (k + 1)) + h["eps"]
            p64[i] = p64[i] * (1 - h["lr"] * h["weight_decay"]) - h["lr"] / (1 - h["betas"][0] ** (k + 1)) * m64[i] / denom
    e = max(float(np.max(np.abs(p.detach().cpu().numpy() - x))) for p, x in zip(eparams, p64))
    t = max(float(np.max(np.abs(p.detach().cpu().numpy() - x))) for p, x in zip(rparams, p64))
    ulp = float(np.spacing(np.float32(max(float(np.max(np.abs(x))) for x in p64))))
    line = (f"ten steps, max_grad_norm 1, lr {h['lr']:g}: largest |p - p64| engine {e:.3e}, torch.optim.AdamW + clip_grad_norm_ {t:.3e} "
            f"(bound 4 x PyTorch's + 2 ulp = {4 * t + 2 * ulp:.3e}; ulp of the largest parameter {ulp:.3e})")
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "optim_parity.txt"), "w") as fh:
        fh.write("tests/test_gpu_optim.py::test_ten_steps_against_pytorch_and_fp64\n" + line + "\n")
    assert e <= 4 * t + 2 * ulp


# ---- 7. state interchange -----------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["engine_to_torch", "torch_to_engine"])
def test_state_passes_both_ways_between_the_engine_and_torch(direction):
    rng = np.random.default_rng(80)
    grads = [[rng.standard_normal(s).astype(np.float32) for s in SIZES] for _ in range(3)]
    case = OC.make_case("interchange", seed=81)
    first, second = (optim.EngineAdamW, torch.optim.AdamW) if direction == "engine_to_torch" else (torch.optim.AdamW, optim.EngineAdamW)
    a, aparams = _build(case, cls=first)
    for k in range(2):
        for p, g in zip(aparams, grads[k]):
            p.grad = _dev(g)
        a.step()
    b, bparams = _build(dict(case, p=[p.detach().cpu().numpy() for p in aparams]), cls=second)
    b.load_state_dict(copy.deepcopy(a.state_dict()))
    before = _results(a, aparams)
    third = dict(case, name=direction, p=before[0], m=before[1], v=before[2], g=grads[2], step=[3] * len(SIZES))
    for opt, params in ((a, aparams), (b, bparams)):
        for p, g in zip(params, grads[2]):
            p.grad = _dev(g)
        opt.step()
        assert all(float(opt.state[p]["step"]) == 3.0 for p in params)
        _assert_within(third, *_results(opt, params))


# ---- 8. a training step end to end --------------------------------------------------------------------
def test_a_training_step_end_to_end_through_the_dropin():
    diff = synth.make_diffuser(seed=0, num_layers=2).eval()
    diff.engine_grad = True
    B, N = 2, 3
    gen = torch.Generator().manual_seed(90)
    x, noise = torch.randn(B, N, 9, generator=gen).to(DEV), torch.randn(B, N, 9, generator=gen).to(DEV)
    z, t = synth.make_z(B, N).to(DEV), torch.tensor([17, 60], device=DEV)
    da, db = copy.deepcopy(diff).to(DEV), copy.deepcopy(diff).to(DEV)
    for d in (da, db):
        d.p_losses(x, t, z=z, noise=noise)["loss"].mean().backward()
    pa, pb = dict(da.model.named_parameters()), dict(db.model.named_parameters())
    assert len(pa) == 108 - 12 * 6 and all(p.grad is not None for p in pb.values())
    assert [n for n in pa if not torch.equal(pa[n].grad, pb[n].grad)] == []             # the trainer promises it
    names = list(pb)
    kw = dict(lr=1e-4, weight_decay=1e-2)
    ref = torch.optim.AdamW(da.model.parameters(), **kw)
    opt = optim.EngineAdamW(db.model.parameters(), max_grad_norm=1.0, **kw)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 0.5 ** k)

    def case_now(step):
        st = [opt.state.get(pb[n], {}) for n in names]
        zeros = [np.zeros(pb[n].numel(), np.float32) for n in names]
        return dict(name=f"training step {step}", groups=[OC.hp(lr=opt.param_groups[0]["lr"], **{k: v for k, v in kw.items() if k != "lr"})],
                    group=[0] * len(names), step=[step] * len(names), max_norm=1.0,
                    p=[pb[n].detach().cpu().numpy().ravel() for n in names], g=[pb[n].grad.cpu().numpy().ravel() for n in names],
                    m=[s["exp_avg"].cpu().numpy().ravel() if s else z0 for s, z0 in zip(st, zeros)],
                    v=[s["exp_avg_sq"].cpu().numpy().ravel() if s else z0 for s, z0 in zip(st, zeros)])

    def flat(res):
        return tuple([x.ravel() for x in part] for part in res)

    case = case_now(1)
    torch.nn.utils.clip_grad_norm_(da.model.parameters(), 1.0)
    ref.step()
    opt.step()
    _assert_within(case, *flat(_results(opt, [pb[n] for n in names])), opt.grad_norm.item())
    # copy A, PyTorch's pairing: were both inside the bounds of the yardstick (u_abs <= lr at step 1) they would be this close
    far = max(float((pa[n] - pb[n]).detach().abs().max()) / (4 * float(np.spacing(np.float32(pb[n].detach().abs().max().item()))) + 64 * OC.U * kw["lr"])
              for n in names)
    print(f"after one step the engine's parameters are at most {far:.3f} of (4 ulp + 64 2^-24 lr) from PyTorch's")
    assert far <= 1.0
    sched.step()
    assert opt.param_groups[0]["lr"] == 0.5e-4
    case = case_now(2)                                                                   # the same gradients once more, at the halved rate
    opt.step()
    _assert_within(case, *flat(_results(opt, [pb[n] for n in names])), opt.grad_norm.item())
    # the version counters: a backward whose forward saw the parameters before a step is refused
    db.zero_grad(set_to_none=True)
    loss = db.p_losses(x, t, z=z, noise=noise)["loss"].mean()
    for p in pb.values():
        p.grad = torch.zeros_like(p)
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


def test_a_non_conforming_tensor_is_refused_by_name():
    case = OC.make_case("refusals", size_list=[8, 5], seed=95)
    opt, params = _build(case)
    params[1].grad = torch.zeros(5, 2, device=DEV)[:, 0]
    with pytest.raises(ValueError, match="the gradient of parameter 1 of group 0 must be a contiguous float32"):
        opt.step()
    p64 = torch.nn.Parameter(torch.zeros(4, dtype=torch.float64, device=DEV))
    p64.grad = torch.ones_like(p64)
    with pytest.raises(ValueError, match="parameter 0 of group 0 must be a contiguous float32"):
        optim.EngineAdamW([p64]).step()
    with pytest.raises(ValueError, match="gradient 0 must be a contiguous float32"):
        optim.clip_grad_norm_([p64], 1.0)
    assert all(len(opt.state[p]) == 0 or float(opt.state[p]["step"]) == 0.0 for p in params)   # a refused step counts for nobody


def test_the_c_abi_refuses_a_call_beyond_its_capacity_and_names_a_bad_argument():
    lib = _lib.load()
    h = C.c_void_p(None)
    assert lib.pd_optimizer_create(2, 100, C.byref(h)) == 0
    bufs = [torch.ones(64, device=DEV) for _ in range(4)]
    before = [b.clone() for b in bufs]
    norm = torch.full((), -1.0, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(n=1, numel=64, group=0, step=1, n_groups=1, null=None, **hp_kw):
        t = (_lib.pd_optim_tensor * 3)()
        for e in t:
            e.param, e.grad, e.exp_avg, e.exp_avg_sq = (b.data_ptr() for b in bufs)
            e.numel, e.group, e.step = numel, group, step
        if null:
            setattr(t[0], null, None)
        g = (_lib.pd_optim_group * 1)()
        v = dict(dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0), **hp_kw)
        g[0].lr, g[0].beta1, g[0].beta2, g[0].eps, g[0].weight_decay = (v[k] for k in ("lr", "beta1", "beta2", "eps", "weight_decay"))
        return lib.pd_optim_adamw_step(h, t, n, g, n_groups, 1.0, norm.data_ptr(), stream), _lib.last_error()

    try:
        for kw, code, word in ((dict(n=3, numel=8), -2, "max_tensors=2"), (dict(n=2, numel=51), -2, "max_numel_total=100"),
                               (dict(numel=-1), -1, "t[0].numel"), (dict(group=1), -1, "t[0].group"), (dict(group=-1), -1, "t[0].group"),
                               (dict(step=0), -1, "t[0].step"), (dict(beta1=1.0), -1, "g[0].beta1"), (dict(beta2=-0.1), -1, "g[0].beta2"),
                               (dict(lr=-1.0), -1, "g[0].lr"), (dict(eps=-1.0), -1, "g[0].eps"), (dict(weight_decay=-1.0), -1, "g[0].weight_decay"),
                               (dict(null="grad"), -1, "grad=NULL"), (dict(null="exp_avg_sq"), -1, "exp_avg_sq=NULL"), (dict(n_groups=0), -1, "n_groups")):
            rc, msg = call(**kw)
            assert rc == code and word in msg and "pd_optim_adamw_step" in msg, (kw, rc, msg)
        torch.cuda.synchronize()
        assert norm.item() == -1.0 and all(torch.equal(a, b) for a, b in zip(bufs, before))      # refused before anything was launched
        assert call(n=0)[0] == 0 and call(numel=0)[0] == 0                                      # nothing to do is no error: the norm of nothing is 0
        torch.cuda.synchronize()
        assert norm.item() == 0.0 and all(torch.equal(a, b) for a, b in zip(bufs, before))
    finally:
        torch.cuda.synchronize()
        lib.pd_optimizer_destroy(h)
