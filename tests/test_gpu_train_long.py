"""GPU (-m gpu): the trainer at 65 ... 256 frames -- PD_TR_OPT_MAX_FRAMES / PD_TR_OPT_LONG_ATTN (include/pd_engine_train.h) through
PoseTrainer.set_max_frames / set_long_attn and the drop-in's ``engine_grad_max_frames``: the key-tiled attention kernels
pd_tr_lattn_kernel, pd_tr_lattn_bwd_rows_kernel and pd_tr_lattn_bwd_keys_kernel (posediffusion_amd/csrc/pd_train_lattn.h).

Parity is teacher-forced exactly as in tests/test_gpu_train_grad.py and tests/test_gpu_train_dropout.py, with their `_check_case`
functions unchanged: masks differ from float64's on at most 1e-5 of the elements, inputs are drawn as `_inputs_for` does, and
model_out, the loss and every gradient tensor and sub-block lie within 4 x the float32 helper's own distance from float64
(``time_embed.linear.0.weight`` at its recorded 16 x).  Every figure is printed before it is asserted; profiles/train_long_parity.txt
holds them.  The networks are train_dropout_checks.CONFIGS' "two" (the default shape, 2 layers) unless a test says otherwise.

  1. tile edges without dropout: N = 65, 128, 129, 192, 193, 255, 256;
  2. other shapes: head dims 24, 12, 68 and 128, the 8-layer default;
  3. dropout at site 0 alone and at all four sites;
  4. a sharp softmax whose row maxima lie in all three key tiles of N = 130 (precondition asserted on float64 before the engine runs;
     train_long_checks.fit_last_tile says why the last tile's two frames are fitted and not drawn);
  5. N <= 64 through the key-tiled kernels: bitwise the default kernels' outputs and gradients, every tensor (DESIGN 3.9 names no exception);
  6. determinism, and independence of the trainer's capacity and of what its stash held before;
  7. the frame limit and the two options;
  8. the drop-in.
Bounds come from the float32 helper or are exact equalities between two engine runs that the header declares bitwise equal."""
import ctypes as C

import pytest
import torch

from denoiser_cfgs import build_dropin
import train_dropout_checks as D
import train_long_checks as L
import test_gpu_train_dropout as GD
import test_gpu_train_grad as G
from test_gpu_train_grad import DEV, MARGIN, NONDEFAULT, RECORDED_MARGIN, _Net, _inputs
from test_gpu_train_grad_edges import HEAD_DIM_CASES, LIMIT_CFGS
from posediffusion_amd import _lib, host, synth
from posediffusion_amd.schedule import diffusion_buffers
from posediffusion_amd.train import PoseTrainer

pytestmark = pytest.mark.gpu


class _LongNet(_Net):
    """`_Net` whose trainers admit 256 frames"""

    def trainer(self, objective, max_B, max_N):
        tr = super().trainer(objective, max_B, max_N)
        if tr.max_frames != L.MAX_FRAMES:
            tr.set_max_frames(L.MAX_FRAMES)
        return tr


@pytest.fixture(scope="module")
def nets(seeded_diffuser):
    made = {"two": _LongNet(L.make_two()), "small": _LongNet(build_dropin(NONDEFAULT, seed=31)), "default": _LongNet(seeded_diffuser.model)}
    for name, (d, nhead, ff, layers) in D.CONFIGS.items():
        s = made[name].shape
        assert (s["d_model"], s["nhead"], s["dim_ff"], s["num_layers"]) == (d, nhead, ff, layers), name
    yield made
    for n in made.values():
        n.close()


def test_margins_are_the_rule():
    assert MARGIN == 4.0 and RECORDED_MARGIN == {"time_embed.linear.0.weight": 16.0}


# ------------------------------------------------------------------------------------------------ 1. tile edges, no dropout
@pytest.mark.parametrize("B,N,objective,loss_type", L.EDGE_CASES, ids=[f"b{c[0]}n{c[1]}" for c in L.EDGE_CASES])
def test_tile_edges_vs_fp64(nets, B, N, objective, loss_type):
    net = nets["two"]
    G._check_case(net, G._inputs_for(net, B, N), objective, loss_type, label=f"long two ({B}, {N}) {objective} {loss_type}")


# ------------------------------------------------------------------------------------------------ 2. other shapes
def test_small_configuration_at_130_frames(nets):
    net = nets["small"]
    G._check_case(net, G._inputs_for(net, 2, 130), "pred_noise", "l1", label="long small (2, 130)")


HEAD_DIMS = [(HEAD_DIM_CASES[0][0], HEAD_DIM_CASES[0][1]), (HEAD_DIM_CASES[1][0], HEAD_DIM_CASES[1][1]), (LIMIT_CFGS[2], 42)]   # head dims 12, 68, 128


@pytest.mark.parametrize("N", [65, 256])
@pytest.mark.parametrize("cfg,seed", HEAD_DIMS, ids=[f"hd{c.d // c.heads}" for c, _ in HEAD_DIMS])
def test_head_dims_at_65_and_256_frames(cfg, seed, N):
    assert [c.d // c.heads for c, _ in HEAD_DIMS] == [12, 68, 128]
    net = _LongNet(build_dropin(cfg, seed))
    try:
        G._check_case(net, G._inputs_for(net, 1, N), "pred_noise", "l1", label=f"long {cfg.name} (1, {N})")
    finally:
        net.close()


def test_eight_layer_default_at_96_frames(nets):
    net = nets["default"]
    G._check_case(net, G._inputs_for(net, 1, 96), "pred_noise", "l1", label="long default (1, 96)")


# ------------------------------------------------------------------------------------------------ 3. dropout
@pytest.mark.parametrize("case", L.DROPOUT_CASES, ids=[c[0] for c in L.DROPOUT_CASES])
def test_dropout_gradients_vs_fp64(nets, case):
    GD._check_case(nets[case[1]], case)


# ------------------------------------------------------------------------------------------------ 4. sharp softmax across tiles
def test_sharp_softmax_across_key_tiles():
    net = _LongNet(L.make_two(L.SHARP_QK))
    try:
        inp = L.fit_last_tile(net.sd, net.net, _inputs(L.SHARP_B, L.SHARP_N, net.shape["z_dim"], L.SHARP_SEED))
        L.check_sharp_precondition(net.sd, net.net, inp)                     # float64 alone, before the engine runs
        G._check_case(net, inp, "pred_noise", "l1", label=f"long sharp ({L.SHARP_B}, {L.SHARP_N})")
    finally:
        net.close()


# ------------------------------------------------------------------------------------------------ 5. bitwise against the short kernels
@pytest.mark.parametrize("drop", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize("N", L.BITWISE_NS)
def test_key_tiled_kernels_give_the_short_kernels_bits(nets, N, drop):
    net = nets["two"]
    inp = _inputs(3, N)
    kw = dict(L.BITWISE_DROP) if drop else {}
    short = PoseTrainer(dict(net.shape, objective="pred_noise"), diffusion_buffers(), 3, N, device=torch.device(DEV))
    tiled = PoseTrainer(dict(net.shape, objective="pred_noise"), diffusion_buffers(), 3, N, device=torch.device(DEV))
    try:
        tiled.set_long_attn(True)
        assert short.get_option(_lib.PD_TR_OPT_LONG_ATTN) == 0 and tiled.get_option(_lib.PD_TR_OPT_LONG_ATTN) == 1
        a, b = GD._bits(short, net, inp, **kw), GD._bits(tiled, net, inp, **kw)
    finally:
        short.close()
        tiled.close()
    differing = [n for n in a if not torch.equal(a[n], b[n])]
    print(f"bitwise N = {N} dropout {drop}: {len(a)} tensors, differing: {differing}")
    assert not differing
    if N == 1:
        d = net.shape["d_model"]
        for n in b:
            if n.endswith(("in_proj_weight", "in_proj_bias")):
                assert b[n][:2 * d].abs().max().item() == 0.0, n              # one key per softmax row: dS is exactly 0


# ------------------------------------------------------------------------------------------------ 6. determinism and capacity
def test_same_call_twice_is_bitwise(nets):
    net = nets["two"]
    inp = _inputs(2, 130)
    tr = net.trainer("pred_noise", 2, 130)
    for kw in ({}, L.CAPACITY_DROP):
        a, b = GD._bits(tr, net, inp, **kw), GD._bits(tr, net, inp, **kw)
        assert all(torch.equal(a[n], b[n]) for n in a), kw


def test_one_trainer_over_batches_of_changing_shape(nets):
    net = nets["two"]
    big = net.trainer("pred_noise", 4, 256)
    for i, (B, N) in enumerate(L.CAPACITY_BATCHES):
        inp = _inputs(B, N, seed=i)
        kw = L.CAPACITY_DROP if i % 2 == 0 else {}
        got = GD._bits(big, net, inp, **kw)
        fresh = PoseTrainer(dict(net.shape, objective="pred_noise"), diffusion_buffers(), B, N, device=torch.device(DEV), max_frames=L.MAX_FRAMES)
        try:
            want = GD._bits(fresh, net, inp, **kw)
        finally:
            fresh.close()
        differing = [n for n in want if not torch.equal(got[n], want[n])]
        print(f"capacity (4, 256) batch {i} ({B}, {N}) dropout {bool(kw)}: differing {differing}")
        assert not differing
        if i == 1:                                           # a forward whose backward never comes: the next forward takes the stash over
            other = _inputs(2, 200, seed=9)
            big.forward(net.gpu, other["x_start"], other["z"], other["t"], other["noise"], "l1", **L.CAPACITY_DROP)


# ------------------------------------------------------------------------------------------------ 7. limits
def test_frame_limit_and_options(nets):
    net = nets["two"]
    new = lambda B, N, **kw: PoseTrainer(dict(net.shape, objective="pred_noise"), diffusion_buffers(), B, N, device=torch.device(DEV), **kw)    # noqa: E731
    fwd = lambda tr, inp: tr.forward(net.gpu, inp["x_start"], inp["z"], inp["t"], inp["noise"], "l1")      # noqa: E731
    inp65, inp64 = _inputs(1, 65), _inputs(1, 64)
    fresh65, fresh64 = new(1, 65, max_frames=L.MAX_FRAMES), new(1, 64)
    tr, cap257 = new(1, 65), new(1, 257)
    try:
        want65, want64 = GD._bits(fresh65, net, inp65), GD._bits(fresh64, net, inp64)
        assert tr.max_frames == 64
        with pytest.raises(RuntimeError, match=r"code -2.*limit of 64 frames per sequence \(the attention backward holds a sequence in LDS\)"):
            fwd(tr, inp65)                                   # today's message
        assert all(torch.equal(v, want64[k]) for k, v in GD._bits(tr, net, inp64).items())
        lib = _lib.load()
        for option, value, what in ((_lib.PD_TR_OPT_MAX_FRAMES, 63, "PD_TR_OPT_MAX_FRAMES=63"), (_lib.PD_TR_OPT_MAX_FRAMES, 257, "PD_TR_OPT_MAX_FRAMES=257"),
                                    (_lib.PD_TR_OPT_LONG_ATTN, 2, "PD_TR_OPT_LONG_ATTN=2"), (3, 1, "unknown option 3")):
            assert lib.pd_trainer_set_option(tr._h, option, value) == -1 and what in _lib.last_error(), what
            assert tr.max_frames == 64 and tr.get_option(_lib.PD_TR_OPT_LONG_ATTN) == 0
            with pytest.raises(RuntimeError, match="limit of 64 frames"):
                fwd(tr, inp65)
            assert all(torch.equal(v, want64[k]) for k, v in GD._bits(tr, net, inp64).items()), what
        v = C.c_int(0)
        assert lib.pd_trainer_get_option(tr._h, 3, C.byref(v)) == -1 and "unknown option 3" in _lib.last_error()
        tr.set_max_frames(256)
        assert tr.max_frames == 256
        assert all(torch.equal(v, want65[k]) for k, v in GD._bits(tr, net, inp65).items())
        tr.set_max_frames(100)                               # the limit moves both ways on the C side; only host.get_trainer never lowers it
        assert tr.max_frames == 100
        cap257.set_max_frames(256)
        with pytest.raises(RuntimeError, match=r"code -2.*N=257 exceeds the trainer's limit of 256 frames"):
            fwd(cap257, _inputs(1, 257))
        with pytest.raises(RuntimeError, match="no forward is pending"):
            cap257.backward(net.gpu, torch.zeros(1, 257, 9, device=DEV))
        assert all(torch.equal(v, want65[k]) for k, v in GD._bits(cap257, net, inp65).items())
    finally:
        for t in (fresh65, fresh64, tr, cap257):
            t.close()


def test_backward_uses_the_family_its_forward_ran(nets):
    net = nets["two"]
    inp = _inputs(3, 5)
    tr = net.trainer("pred_noise", 3, 5)
    want = GD._bits(tr, net, inp)
    tr.forward(net.gpu, inp["x_start"], inp["z"], inp["t"], inp["noise"], "l1")
    tr.set_long_attn(True)                                   # between the two calls: the pending backward stays with the short kernels
    grads = tr.backward(net.gpu, torch.full((3, 5, 9), 1.0 / (3 * 5 * 9), device=DEV))
    tr.set_long_attn(False)
    assert all(torch.equal(g.cpu(), want[n]) for n, g in grads.items())


# ------------------------------------------------------------------------------------------------ 8. the drop-in
def test_dropin_engine_grad_max_frames():
    diff = synth.make_diffuser(seed=0, num_layers=2)
    synth.randomize_norm_and_bias_(diff.model)
    diff = diff.to(DEV)
    diff.eval()
    diff.engine_grad = True
    B, N = 2, 65
    inp = {k: v.to(DEV) for k, v in _inputs(B, N).items()}
    call = lambda: diff.p_losses(inp["x_start"], inp["t"], z=inp["z"], noise=inp["noise"])      # noqa: E731
    with pytest.raises(RuntimeError, match=r"limit of 64 frames.*engine_grad_max_frames = 65"):
        call()
    diff.engine_grad_max_frames = 256
    r = call()
    r["loss"].sum().backward()
    got = {n: p.grad.clone().cpu() for n, p in diff.model.named_parameters()}
    net = _LongNet(diff.model, diff)
    try:
        tr = net.trainer("pred_noise", B, N)
        out = tr.forward(net.gpu, inp["x_start"], inp["z"], inp["t"], inp["noise"], "l1")
        want = tr.backward(net.gpu, torch.ones(B, N, 9, device=DEV))
    finally:
        net.close()
    assert torch.equal(r["loss"].detach(), out["loss"])
    assert all(torch.equal(got[n], want[n].cpu()) for n in got)
    assert host.get_trainer(diff.model, diff, B, N).max_frames == 256       # a later call at the default never lowers the cached trainer's limit
    diff.train()
    diff.engine_dropout = True

    def step():
        torch.manual_seed(5)
        diff.model.zero_grad(set_to_none=True)
        rr = call()
        rr["loss"].sum().backward()
        return rr["loss"].detach().clone(), {n: p.grad.clone() for n, p in diff.model.named_parameters()}

    l1, g1 = step()
    l2, g2 = step()
    assert torch.equal(l1, l2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    assert not torch.equal(l1, r["loss"].detach())
    host.get_trainer(diff.model, diff, B, N).close()
