"""GPU (-m gpu): the trainer's dropout -- pd_train_forward_dropout / pd_train_backward (include/pd_engine_train.h) through
PoseTrainer.forward(dropout_p=..., dropout_sites=..., seed=..., step=...) and the drop-in opt-in ``GaussianDiffusion.engine_dropout``.

Parity is teacher-forced exactly as in tests/test_gpu_train_grad.py, against tests/train_dropout_checks.py (train_checks' float64 /
float32 p_losses with the four sites applied from the host mirror of the mask definition).  Every case
  1. runs the forward with dropout, 2. reads the stashed FF activations (pd_train_debug_relu: post-dropout, so ``> 0`` is "ReLU passed
  and kept") and the loss signs, 3. runs pd_train_backward with g_loss = 1 / (B N 9), then checks
  * the MASK condition: the engine's combined masks equal ``(float64 pre-activation > 0) and keep_mask`` except on at most 1e-5 of the
    elements, its loss signs differ in none, and the stash is within 4 x own of relu(a64) keep scale;
  * PARITY: model_out, loss and every gradient tensor and sub-block (train_checks.block_misses) within 4 x the float32 helper's own
    distance from float64, same masks forced; where float64's gradient is identically zero (N = 1: q and k rows) the engine's is too.
``time_embed.linear.0.weight`` keeps the 16 x margin on record for it (profiles/train_grad_parity.txt, restated with this suite's figures
in profiles/train_dropout_parity.txt): its cause -- one-ulp differences of 3 of the 128 fp32 frequencies -- does not involve dropout.
Every figure is printed before it is asserted.  The cases and their seeds are train_dropout_checks.GPU_CASES; the keep rate of each of
their masks is checked on the CPU (tests/test_train_dropout_cpu.py).

Inputs are drawn like test_gpu_train_grad._inputs_for: a case of fewer than 1e5 activations admits no differing mask, so its draw is the
first for which the float64 helper WITH the case's dropout has no ReLU input inside the band u sqrt(d_model) x the layer's largest."""
import pytest
import torch

from denoiser_cfgs import build_dropin
from oracle import pd_oracle as O
import train_checks as TC
import train_dropout_checks as D
from posediffusion_amd import host, synth
from test_gpu_train_grad import DEV, MARGIN, NONDEFAULT, RECORDED_MARGIN, _Net, _inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nets(seeded_diffuser):
    two = synth.make_diffuser(seed=0, num_layers=2)
    synth.randomize_norm_and_bias_(two.model)
    made = {"two": _Net(two.model), "small": _Net(build_dropin(NONDEFAULT, seed=31)), "default": _Net(seeded_diffuser.model)}
    for name, (d, nhead, ff, layers) in D.CONFIGS.items():
        s = made[name].shape
        assert (s["d_model"], s["nhead"], s["dim_ff"], s["num_layers"]) == (d, nhead, ff, layers), name
    yield made
    for n in made.values():
        n.close()


def _pre64(net, inp, sites, drop):
    with torch.no_grad():
        sd = {k: v.double() for k, v in net.sd.items()}
        x_t = TC.q_sample(inp["x_start"].double(), inp["noise"].double(), inp["t"], O.diffusion_tables(dtype=torch.float64))
        return D.denoiser_forward_dropout(sd, net.net, x_t, inp["t"], inp["z"].double(), sites, drop)[1]["pre"]


def _inputs_for(net, B, N, sites, drop):
    zdim, d = net.shape["z_dim"], net.shape["d_model"]
    total = B * N * (net.net.layers * net.shape["dim_ff"] + net.shape["mlp_hidden"])
    for seed in range(16):
        inp = _inputs(B, N, zdim, seed)
        if 1e-5 * total >= 1.0:
            return inp
        if all(a.abs().min().item() > 2.0 ** -24 * d ** 0.5 * a.max().item() for a in _pre64(net, inp, sites, drop)):
            return inp
    raise AssertionError("no well-posed draw among 16 seeds")


def _keep_ff(net, B, N, l, sites, drop):
    """keep_mask of the FF site of layer l as a [B N, ff] bool tensor (all True where the site is off or the layer is _last)"""
    ff = net.shape["dim_ff"] if l < net.net.layers else net.shape["mlp_hidden"]
    if l >= net.net.layers or not sites & D.FF or drop[0] == 0.0:
        return torch.ones(B * N, ff, dtype=torch.bool)
    return torch.from_numpy(D.keep_mask(B * N, ff, l, 2, drop[1], drop[2], drop[0]))


def _engine_pass(tr, net, inp, loss_type, p, sites, seed, step):
    B, N, _ = inp["x_start"].shape
    out = tr.forward(net.gpu, inp["x_start"], inp["z"], inp["t"], inp["noise"], loss_type, dropout_p=p, dropout_sites=sites, seed=seed, step=step)
    tr.check_async()
    relu = [tr.debug_relu(l).cpu() for l in range(net.net.layers + 1)]
    grads = tr.backward(net.gpu, torch.full((B, N, 9), 1.0 / (B * N * 9), device=DEV))
    return {k: v.cpu() for k, v in out.items()}, relu, {k: v.cpu() for k, v in grads.items()}


def _check_case(net, case):
    label, _, B, N, p, sites, seed, step, objective, loss_type = case
    drop = (p, seed, step)
    inp = _inputs_for(net, B, N, sites, drop)
    tr = net.trainer(objective, B, N)
    out, relu, grads = _engine_pass(tr, net, inp, loss_type, p, sites, seed, step)
    target = inp["noise"] if objective == "pred_noise" else inp["x_start"]
    masks_e = [r > 0 for r in relu]
    signs_e = torch.sign(out["model_out"] - target)
    args = (net.sd, net.net, inp, objective, loss_type, p, sites, seed, step)
    own64 = D.loss_and_grads_dropout(*args, want=[])
    r64 = D.loss_and_grads_dropout(*args, masks=masks_e, signs=signs_e)
    r32 = D.loss_and_grads_dropout(*args, masks=masks_e, signs=signs_e, dtype=torch.float32)
    total = sum(m.numel() for m in masks_e)
    ndiff, problems = 0, []
    fscale = D.scale_of(p) if sites & D.FF else 1.0
    for l, (me, a64, a32, post) in enumerate(zip(masks_e, own64["pre"], r32["pre"], relu)):
        keep = _keep_ff(net, B, N, l, sites, drop)
        ks = keep.double() * (fscale if l < net.net.layers else 1.0)
        a64 = a64.reshape(me.shape)
        want = a64.clamp_min(0) * ks
        scale = max(want.abs().max().item(), 1e-300)
        own = (a32.reshape(me.shape).double().clamp_min(0) * ks - want).abs().max().item() / scale
        e = (post.double() - want).abs().max().item() / scale
        differ = me != ((a64 > 0) & keep)
        ndiff += int(differ.sum())
        print(f"{label} relu {l}: stash {e:.3e} own {own:.3e}; {int(differ.sum())} of {me.numel()} differ from (a64 > 0) and keep; kept {keep.double().mean():.4f}")
        if e > MARGIN * own:
            problems.append(("stash", l, e, own))
    print(f"{label} masks: {ndiff} of {total} differ; loss signs differing: {int((signs_e != own64['signs']).sum())}")
    assert ndiff <= 1e-5 * total, (ndiff, total)
    assert torch.equal(signs_e.double(), own64["signs"])
    for k in ("model_out", "loss"):
        e, own = TC.grad_dist(out[k], r64[k]), TC.grad_dist(r32[k], r64[k])
        print(f"{label} {k}: engine {e:.3e} own {own:.3e}")
        if e > MARGIN * own:
            problems.append((k, e, own))
    worst = (0.0, "", 0.0, 0.0)
    d, zdim = net.shape["d_model"], net.shape["z_dim"]
    for n in list(net.sd) + ["z"]:
        g64, g = r64["grads"][n], grads[n]
        assert torch.isfinite(g).all(), n
        if N == 1 and n.endswith(("in_proj_weight", "in_proj_bias")):
            assert g64[:2 * d].abs().max().item() == 0.0 and g[:2 * d].abs().max().item() == 0.0, n      # one key per softmax row: dS is exactly 0
        if g64.abs().max().item() == 0.0:
            assert g.abs().max().item() == 0.0, (n, "float64 gradient is identically zero")
            continue
        e, own = TC.grad_dist(g, g64), TC.grad_dist(r32["grads"][n], g64)
        if e / max(own, 1e-30) > worst[0]:
            worst = (e / max(own, 1e-30), n, e, own)
        if e > RECORDED_MARGIN.get(n, MARGIN) * own:
            print(f"{label} PARITY MISS {n}: engine {e:.3e} own {own:.3e} ({e / own:.2f} x)")
            problems.append(("parity", n, e, own))
        for bn, be, bown in TC.block_misses(n, g, r32["grads"][n], g64, d, zdim, MARGIN, RECORDED_MARGIN):
            print(f"{label} BLOCK MISS {bn}: engine {be:.3e} own {bown:.3e}")
            problems.append(("block", bn, be, bown))
    print(f"{label} parity: worst engine / own = {worst[0]:.2f} ({worst[1]}: engine {worst[2]:.3e}, own {worst[3]:.3e})")
    assert not problems, problems
    return inp, out, relu, own64


@pytest.mark.parametrize("case", D.GPU_CASES, ids=[c[0] for c in D.GPU_CASES])
def test_dropout_gradients_vs_fp64(nets, case):
    net = nets[case[1]]
    B, N, p, sites, seed, step = case[2], case[3], case[4], case[5], case[6], case[7]
    inp, out, relu, own64 = _check_case(net, case)
    if sites & D.FF:
        # the zeros of the stash among the activations float64 passes are exactly the dropped elements (no flip was admitted above
        # unless the case has 1e5 activations; there the elements inside the rounding band are left out)
        d = net.shape["d_model"]
        for l in range(net.net.layers):
            a64 = own64["pre"][l].reshape(relu[l].shape)
            sure = a64 > 2.0 ** -24 * d ** 0.5 * a64.max().item()
            keep = _keep_ff(net, B, N, l, sites, (p, seed, step))
            assert torch.equal((relu[l] == 0)[sure], ~keep[sure]), l
            print(f"{case[0]} layer {l}: {int((relu[l] == 0)[sure].sum())} of {int(sure.sum())} passed activations are dropped, as keep_mask says")


def _bits(tr, net, inp, loss_type="l1", **kw):
    B, N, _ = inp["x_start"].shape
    out = tr.forward(net.gpu, inp["x_start"], inp["z"], inp["t"], inp["noise"], loss_type, **kw)
    grads = tr.backward(net.gpu, torch.full((B, N, 9), 1.0 / (B * N * 9), device=DEV))
    tr.check_async()
    return {**{"out." + k: v.cpu() for k, v in out.items()}, **{k: v.cpu() for k, v in grads.items()}}


def test_no_dropout_calls_are_bitwise_the_plain_forward_and_backward(nets):
    net = nets["two"]
    inp = _inputs(3, 5)
    tr = net.trainer("pred_noise", 3, 5)
    plain = _bits(tr, net, inp)
    real = tr.lib.pd_train_forward_dropout
    # p = 0.3 with sites = 0 reaches the C entry (PoseTrainer routes only p == 0 to pd_train_forward); p = 0 is sent there by hand below
    zero_sites = _bits(tr, net, inp, dropout_p=0.3, dropout_sites=0, seed=9, step=1)
    zero_p = _bits(tr, net, inp, dropout_p=0.0, dropout_sites=D.ALL, seed=9, step=1)
    for k in plain:
        assert torch.equal(plain[k], zero_sites[k]), (k, "sites = 0, p = 0.3")
        assert torch.equal(plain[k], zero_p[k]), (k, "p = 0")
    # p = 0 through the C entry as well
    B, N = 3, 5
    live = tr._live(net.gpu)
    w = tr._weights_struct(live)
    import ctypes as C
    bufs = {k: torch.empty(B, N, 9, device=DEV) for k in ("loss", "x0", "xt", "mo")}
    dev = {k: inp[k].to(DEV).contiguous() for k in ("x_start", "z", "noise")}
    t = inp["t"].to(DEV)
    rc = real(tr._h, C.byref(w), dev["x_start"].data_ptr(), dev["z"].data_ptr(), t.data_ptr(), dev["noise"].data_ptr(), B, N, 1, 0.0, D.ALL, 9, 1,
              bufs["loss"].data_ptr(), bufs["x0"].data_ptr(), bufs["xt"].data_ptr(), bufs["mo"].data_ptr(), tr._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(bufs["mo"].cpu(), plain["out.model_out"]) and torch.equal(bufs["loss"].cpu(), plain["out.loss"])
    tr._pending = (B, N)                                     # consume the stash of the raw call
    tr.backward(net.gpu, torch.zeros(B, N, 9, device=DEV))


def test_bitwise_reproducible_independent_of_capacity_and_keyed_by_seed_and_step(nets):
    net = nets["two"]
    inp = _inputs(7, 19)
    exact, big = net.trainer("pred_noise", 7, 19), net.trainer("pred_noise", 64, 64)
    kw = dict(dropout_p=0.1, dropout_sites=D.ALL, seed=(3 << 32) | 5, step=2)
    a, b, c = _bits(exact, net, inp, **kw), _bits(exact, net, inp, **kw), _bits(big, net, inp, **kw)
    for n in a:
        assert torch.equal(a[n], b[n]), (n, "second run")
        assert torch.equal(a[n], c[n]), (n, "capacity (64, 64)")
    plain = _bits(exact, net, inp)
    assert not torch.equal(a["out.model_out"], plain["out.model_out"])
    for other in (dict(kw, step=3), dict(kw, seed=(3 << 32) | 6), dict(kw, seed=(4 << 32) | 5)):
        assert not torch.equal(_bits(exact, net, inp, **other)["out.model_out"], a["out.model_out"]), other
    after = _bits(exact, net, inp)                           # dropout leaves nothing behind on the trainer
    for n in plain:
        assert torch.equal(plain[n], after[n]), n


def test_bad_arguments_are_refused_and_leave_a_usable_trainer(nets):
    net = nets["two"]
    inp = _inputs(3, 5)
    tr = net.trainer("pred_noise", 3, 5)
    ref = _bits(tr, net, inp, dropout_p=0.1, seed=1)
    for kw, msg in ((dict(dropout_p=1.0), "argument p="), (dict(dropout_p=float("nan")), "argument p="), (dict(dropout_p=-0.5), "argument p="),
                    (dict(dropout_p=0.1, dropout_sites=16), "argument sites="), (dict(dropout_p=0.0, dropout_sites=32), "argument sites=")):
        with pytest.raises(RuntimeError, match=r"code -1.*" + msg):
            tr.forward(net.gpu, inp["x_start"], inp["z"], inp["t"], inp["noise"], "l1", **kw)
        with pytest.raises(RuntimeError, match="no forward is pending"):
            tr.backward(net.gpu, torch.zeros(3, 5, 9, device=DEV))
    again = _bits(tr, net, inp, dropout_p=0.1, seed=1)
    assert all(torch.equal(ref[k], again[k]) for k in ref)


def test_dropin_engine_dropout_trains_the_default_diffuser_as_built():
    diff = synth.make_diffuser(seed=0)
    synth.randomize_norm_and_bias_(diff.model)
    diff = diff.to(DEV)
    inp = {k: v.to(DEV) for k, v in _inputs(3, 5).items()}
    call = lambda: diff.p_losses(inp["x_start"], inp["t"], z=inp["z"], noise=inp["noise"])      # noqa: E731
    diff.engine_grad = True
    diff.eval()
    ev = call()
    ev["loss"].mean().backward()
    g_eval = {n: p.grad.clone() for n, p in diff.model.named_parameters()}
    diff.model.zero_grad(set_to_none=True)
    diff.train()
    with pytest.raises(RuntimeError, match="dropout"):      # the first opt-in alone still refuses
        call()
    diff.engine_dropout = True
    assert diff._dropout_p() == 0.1

    def step(seed=None):
        if seed is not None:
            torch.manual_seed(seed)
        diff.model.zero_grad(set_to_none=True)
        r = call()
        assert r["loss"].requires_grad and sorted(r) == ["loss", "noise", "t", "x_0_pred", "x_t"]
        r["loss"].mean().backward()
        grads = {n: p.grad.clone() for n, p in diff.model.named_parameters()}
        assert all(g is not None and torch.isfinite(g).all() for g in grads.values())
        assert all(g.abs().max() > 0 for g in grads.values())
        return r["loss"].detach().clone(), grads

    l1, g1 = step(5)
    l2, g2 = step()                                         # consecutive calls draw another seed
    l3, g3 = step(5)
    assert torch.equal(l1, l3) and all(torch.equal(g1[n], g3[n]) for n in g1)
    assert not torch.equal(l1, l2) and not torch.equal(l1, ev["loss"])
    rel = ((l1 - ev["loss"]).abs().max() / ev["loss"].abs().max()).item()
    print(f"dropout 0.1 moves the loss by {rel:.3e} of its maximum")
    assert 1e-3 < rel < 10.0
    diff.eval()                                             # .eval(): today's path, bit for bit, whatever engine_dropout says
    diff.model.zero_grad(set_to_none=True)
    on = call()
    on["loss"].mean().backward()
    assert torch.equal(on["loss"], ev["loss"]) and all(torch.equal(p.grad, g_eval[n]) for n, p in diff.model.named_parameters())
    diff.engine_dropout = False
    diff.model.zero_grad(set_to_none=True)
    off = call()
    off["loss"].mean().backward()
    assert torch.equal(off["loss"], ev["loss"]) and all(torch.equal(p.grad, g_eval[n]) for n, p in diff.model.named_parameters())
    host.get_trainer(diff.model, diff, 3, 5).close()
