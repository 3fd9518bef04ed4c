"""GPU (-m gpu): gradients through model_out and x_0_pred on the trainer -- pd_train_backward_ex (include/pd_engine_train.h) through
``PoseTrainer.backward(..., g_model_out=, g_x0_pred=)`` -- on the default shape with 2 encoder layers (train_long_checks.make_two).

  BITWISE   the row vector that enters _last.3 is the sum of the PRESENT terms g_loss dl, g_model_out, k_b g_x0_pred, each a single fp32
            product, so on every parameter gradient and dz
              _ex(g_loss)              == pd_train_backward(g_loss)
              _ex(g_model_out = G dl)  == pd_train_backward(G)        dl = sign(d) / 2 d in torch fp32 from model_out and the target
              _ex(g_x0_pred = G)       == _ex(g_model_out = -c[t] G)  under pred_noise, c = the fp32 sqrt_recipm1_alphas_cumprod
              _ex(g_x0_pred = G)       == _ex(g_model_out = G)        under pred_x0
            on case b3n5 (15 rows: not a multiple of the tail's 4 rows per block), (1, 1) and a padded (3, 7) with counts (7, 1, 4).
            Each side runs its own forward (the forward is deterministic).
  FLOAT64   all three upstreams together (draw_upstream, three seeds) against tests/train_outputs_checks.py with the engine's ReLU masks
            and l1 signs forced: every parameter gradient, dz and every train_checks.grad_blocks block within 4 x the float32
            restatement's own distance (16 x for ``time_embed.linear.0.weight``, test_gpu_train_grad.RECORDED_MARGIN), exact zeros where
            float64's are zero; x_0_pred and model_out themselves by the same rule.  Once more after pd_train_forward_dropout (p = 0.1,
            all sites) and once at (2, 65) with max_frames = 65 (the key-tiled attention).
  RAGGED    padding rows of g_model_out and g_x0_pred filled with NaN change no bit; each slot's dz is bitwise its sequence run alone.
  ERRORS    no upstream at all, g_x0_pred without the recip tables (before anything is launched: the stash stays), a second backward.
Every figure is printed before it is asserted; profiles/train_outputs_parity.txt records the worst ones."""
import ctypes as C

import pytest
import torch

from p_losses_cases import inputs as case_inputs
import test_gpu_train_grad as G
import train_checks as TC
import train_dropout_checks as TD
import train_long_checks as L
import train_outputs_checks as TO
from posediffusion_amd import _lib
from posediffusion_amd import train as T
from posediffusion_amd.schedule import diffusion_buffers
from posediffusion_amd.train import PoseTrainer

pytestmark = pytest.mark.gpu
DEV = G.DEV
MARGIN, RECORDED_MARGIN = G.MARGIN, G.RECORDED_MARGIN
COUNTS = (7, 1, 4)
BATCHES = {"b3n5": (lambda: case_inputs(1), None), "b1n1": (lambda: case_inputs(0), None), "ragged_b3n7": (lambda: G._inputs(3, 7), COUNTS)}
DROP = dict(dropout_p=0.1, dropout_sites=TD.ALL, seed=61, step=2)


@pytest.fixture(scope="module")
def two():
    n = G._Net(L.make_two())
    yield n
    n.close()


def _forward(tr, net, inp, loss_type, counts=None, drop=None):
    out = tr.forward(net.gpu, inp["x_start"], inp["z"], inp["t"], inp["noise"], loss_type, n_frames=counts, **(drop or {}))
    tr.check_async()
    return out


def _cpu(d):
    return {k: v.cpu() for k, v in d.items()}


def _run(tr, net, inp, loss_type, counts=None, drop=None, **ups):
    """its own forward, then ``PoseTrainer.backward`` with the upstreams ``ups`` (CPU tensors) -> every gradient and dz on the CPU"""
    _forward(tr, net, inp, loss_type, counts, drop)
    return _cpu(tr.backward(net.gpu, **{k: v.to(DEV) for k, v in ups.items()}))


def _backward_ex(tr, net, g_loss=None, g_model_out=None, g_x0_pred=None):
    """pd_train_backward_ex itself on the pending stash (``PoseTrainer.backward`` sends g_loss alone to pd_train_backward) -> (rc, grads)"""
    B, N = tr._pending
    live = tr._live(net.gpu)
    grads = {n: torch.empty_like(live[n]) for n in tr.names}
    grads["z"] = torch.empty(B, N, int(tr.shape["z_dim"]), device=DEV)
    g = _lib.pd_weight_grads()
    T._fill(g, tr.num_layers, lambda n: grads[n].data_ptr())
    w = tr._weights_struct(live)
    ups = [None if u is None else u.to(device=DEV, dtype=torch.float32).contiguous() for u in (g_loss, g_model_out, g_x0_pred)]
    rc = tr.lib.pd_train_backward_ex(tr._h, C.byref(w), *(None if u is None else u.data_ptr() for u in ups), C.byref(g), grads["z"].data_ptr(),
                                     tr._stream())
    torch.cuda.synchronize()
    if rc == 0:
        tr._pending = None
    return rc, _cpu(grads)


def _assert_same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    differ = [n for n in a if not torch.equal(a[n], b[n])]
    assert differ == [], (what, differ)
    assert all(torch.isfinite(v).all() for v in a.values()), what
    assert any(v.abs().max() > 0 for v in a.values()), (what, "every gradient is zero")


@pytest.mark.parametrize("objective", ["pred_noise", "pred_x0"])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_single_terms_are_single_fp32_products(two, batch, objective):
    make, counts = BATCHES[batch]
    inp = make()
    B, N, _ = inp["x_start"].shape
    tr = two.trainer(objective, B, N)
    Gu = TO.draw_upstream(B, N, 4)
    target = (inp["noise"] if objective == "pred_noise" else inp["x_start"]).to(DEV)
    for loss_type in ("l1", "l2"):
        plain = _run(tr, two, inp, loss_type, counts, g_loss=Gu)                                   # pd_train_backward
        _forward(tr, two, inp, loss_type, counts)
        rc, ex = _backward_ex(tr, two, g_loss=Gu)
        assert rc == 0, _lib.last_error()
        _assert_same_bits(ex, plain, f"{batch} {objective} {loss_type}: _ex(g_loss) vs pd_train_backward")
        out = _forward(tr, two, inp, loss_type, counts)
        d = out["model_out"] - target
        dl = torch.sign(d) if loss_type == "l1" else 2.0 * d
        via_mo = _cpu(tr.backward(two.gpu, g_model_out=Gu.to(DEV) * dl))
        _assert_same_bits(via_mo, plain, f"{batch} {objective} {loss_type}: _ex(g_model_out = G dl) vs pd_train_backward(G)")
    via_x0 = _run(tr, two, inp, "l1", counts, g_x0_pred=Gu)
    if objective == "pred_noise":
        c = diffusion_buffers()["sqrt_recipm1_alphas_cumprod"].to(device=DEV, dtype=torch.float32)
        k = (-c[inp["t"].to(DEV)]).reshape(B, 1, 1)
        same = _cpu(_run_dev(tr, two, inp, counts, k * Gu.to(DEV)))
        assert (k.abs() != 1).all()
    else:
        same = _run(tr, two, inp, "l1", counts, g_model_out=Gu)
    _assert_same_bits(via_x0, same, f"{batch} {objective}: _ex(g_x0_pred = G) vs _ex(g_model_out = k G)")
    plain = _run(tr, two, inp, "l1", counts, g_loss=Gu)
    assert any(not torch.equal(via_x0[n], plain[n]) for n in plain)                                 # (another function than the loss's)


def _run_dev(tr, net, inp, counts, g_mo_dev):
    _forward(tr, net, inp, "l1", counts)
    return tr.backward(net.gpu, g_model_out=g_mo_dev)


def _check_vs_fp64(net, tr, inp, objective, loss_type, label, drop=None):
    B, N, _ = inp["x_start"].shape
    ups = dict(g_loss=TO.draw_upstream(B, N, 1), g_model_out=TO.draw_upstream(B, N, 2), g_x0_pred=TO.draw_upstream(B, N, 3))
    out = _cpu(_forward(tr, net, inp, loss_type, None, drop))
    masks = [tr.debug_relu(l).cpu() > 0 for l in range(net.net.layers + 1)]
    grads = _cpu(tr.backward(net.gpu, **{k: v.to(DEV) for k, v in ups.items()}))
    target = inp["noise"] if objective == "pred_noise" else inp["x_start"]
    signs = torch.sign(out["model_out"] - target)
    d4 = None if drop is None else (drop["dropout_p"], drop["dropout_sites"], drop["seed"], drop["step"])
    r64 = TO.outputs_and_grads(net.sd, net.net, inp, objective, loss_type, **ups, masks=masks, signs=signs, drop=d4)
    r32 = TO.outputs_and_grads(net.sd, net.net, inp, objective, loss_type, **ups, masks=masks, signs=signs, drop=d4, dtype=torch.float32)
    problems, worst = [], (0.0, "", 0.0, 0.0)
    for k in ("model_out", "x_0_pred"):
        e, own = TC.grad_dist(out[k], r64[k]), TC.grad_dist(r32[k], r64[k])
        print(f"{label} {k}: engine {e:.3e} own {own:.3e}")
        if e > MARGIN * own:
            problems.append((k, e, own))
    d, zdim = net.shape["d_model"], net.shape["z_dim"]
    for n in list(net.sd) + ["z"]:
        g64, g, g32 = r64["grads"][n], grads[n], r32["grads"][n]
        assert torch.isfinite(g).all(), n
        if g64.abs().max().item() == 0.0:
            assert g.abs().max().item() == 0.0, (n, "float64 gradient is identically zero")
            continue
        e, own = TC.grad_dist(g, g64), TC.grad_dist(g32, g64)
        if e / max(own, 1e-30) > worst[0]:
            worst = (e / max(own, 1e-30), n, e, own)
        if e > RECORDED_MARGIN.get(n, MARGIN) * own:
            print(f"{label} PARITY MISS {n}: engine {e:.3e} own {own:.3e} ({e / max(own, 1e-30):.2f} x)")
            problems.append(("parity", n, e, own))
        for bn, be, bown in TC.block_misses(n, g, g32, g64, d, zdim, MARGIN, RECORDED_MARGIN):
            print(f"{label} BLOCK MISS {bn}: engine {be:.3e} own {bown:.3e}")
            problems.append(("block", bn, be, bown))
    print(f"{label} parity: worst engine / own = {worst[0]:.2f} ({worst[1]}: engine {worst[2]:.3e}, own {worst[3]:.3e})")
    assert not problems, problems


@pytest.mark.parametrize("objective,loss_type", [("pred_noise", "l1"), ("pred_noise", "l2"), ("pred_x0", "l1"), ("pred_x0", "l2")])
def test_three_upstreams_vs_fp64_b3n5(two, objective, loss_type):
    _check_vs_fp64(two, two.trainer(objective, 3, 5), case_inputs(1), objective, loss_type, f"b3n5 {objective} {loss_type}")


def test_three_upstreams_vs_fp64_b1n1(two):
    _check_vs_fp64(two, two.trainer("pred_noise", 3, 5), case_inputs(0), "pred_noise", "l1", "b1n1 pred_noise l1")


def test_three_upstreams_vs_fp64_after_dropout(two):
    _check_vs_fp64(two, two.trainer("pred_noise", 3, 5), case_inputs(1), "pred_noise", "l1", "b3n5 dropout 0.1", drop=DROP)


def test_three_upstreams_vs_fp64_at_65_frames(two):
    tr = PoseTrainer(dict(two.shape, objective="pred_noise"), diffusion_buffers(), 2, 65, device=torch.device(DEV), max_frames=65)
    two._trainers["n65"] = tr                                       # closed with the fixture
    _check_vs_fp64(two, tr, G._inputs(2, 65), "pred_noise", "l1", "b2n65 key-tiled")


@pytest.mark.parametrize("objective", ["pred_noise", "pred_x0"])
def test_ragged_padding_is_never_read_and_slots_are_their_sequences_alone(two, objective):
    inp = G._inputs(3, 7)
    B, N = 3, 7
    tr = two.trainer(objective, B, N)
    ups = dict(g_loss=TO.draw_upstream(B, N, 1), g_model_out=TO.draw_upstream(B, N, 2), g_x0_pred=TO.draw_upstream(B, N, 3))
    clean = _run(tr, two, inp, "l1", COUNTS, **ups)
    nan = {k: v.clone() for k, v in ups.items()}
    for b, n in enumerate(COUNTS):
        for k in nan:
            nan[k][b, n:] = float("nan")
    _assert_same_bits(_run(tr, two, inp, "l1", COUNTS, **nan), clean, f"{objective}: NaN at the padding rows of every upstream")
    for b, n in enumerate(COUNTS):
        assert (clean["z"][b, n:] == 0).all() and not torch.signbit(clean["z"][b, n:]).any(), ("dz padding", b)
        alone_inp = {"x_start": inp["x_start"][b:b + 1, :n], "noise": inp["noise"][b:b + 1, :n], "z": inp["z"][b:b + 1, :n], "t": inp["t"][b:b + 1]}
        alone = _run(tr, two, alone_inp, "l1", None, **{k: v[b:b + 1, :n] for k, v in ups.items()})
        assert torch.equal(alone["z"][0], clean["z"][b, :n]), (objective, "dz of slot", b)


def test_refusals_leave_the_stash_and_a_usable_trainer(two):
    inp = case_inputs(1)
    tr = two.trainer("pred_noise", 3, 5)
    Gu = TO.draw_upstream(3, 5, 4)
    want = _run(tr, two, inp, "l1", g_loss=Gu)
    _forward(tr, two, inp, "l1")
    with pytest.raises(RuntimeError, match=r"pd_train_backward_ex failed \(code -1\).*all NULL"):
        tr.backward(two.gpu)
    rc, _ = _backward_ex(tr, two)
    assert rc == -1 and "pd_train_backward_ex" in _lib.last_error() and "all NULL" in _lib.last_error()
    _assert_same_bits(_cpu(tr.backward(two.gpu, Gu.to(DEV))), want, "the stash survived the refusals")
    with pytest.raises(RuntimeError, match=r"code -4.*no forward is pending"):                       # a stash is consumed once
        tr.backward(two.gpu, g_model_out=Gu.to(DEV))
    tr._pending = (3, 5)                                                                             # the C entry itself
    rc, _ = _backward_ex(tr, two, g_x0_pred=Gu)
    tr._pending = None
    assert rc == -4 and "pd_train_backward_ex: no forward is pending" in _lib.last_error()
    # a trainer created without the recip tables: x_0_pred is unavailable under pred_noise, and so is its upstream
    bufs = {k: v for k, v in diffusion_buffers().items() if k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")}
    bare = PoseTrainer(dict(two.shape, objective="pred_noise"), bufs, 3, 5, device=torch.device(DEV))
    two._trainers["bare"] = bare
    dev = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    loss, mo = torch.empty(3, 5, 9, device=DEV), torch.empty(3, 5, 9, device=DEV)
    w = bare._weights_struct(bare._live(two.gpu))
    assert bare.lib.pd_train_forward(bare._h, C.byref(w), dev["x_start"].data_ptr(), dev["z"].data_ptr(), dev["t"].data_ptr(), dev["noise"].data_ptr(),
                                     3, 5, 1, loss.data_ptr(), None, None, mo.data_ptr(), bare._stream()) == 0, _lib.last_error()
    bare._pending = (3, 5)
    with pytest.raises(RuntimeError, match=r"pd_train_backward_ex failed \(code -4\).*g_x0_pred under pred_noise needs sqrt_recip"):
        bare.backward(two.gpu, g_x0_pred=Gu.to(DEV))
    assert bare._pending == (3, 5)                                                                   # nothing was launched: the stash is still pending
    _assert_same_bits(_cpu(bare.backward(two.gpu, Gu.to(DEV))), want, "the bare trainer's stash after the refusal")
