"""GPU (-m gpu): the trainer's backward (include/pd_engine_train.h) where tests/test_gpu_train_grad.py does not reach, with that file's
method (teacher-forced float64 yardstick, mask condition, 4 x own per tensor AND per sub-block, exact zeros where float64's are) and
its helpers:

  A. a non-uniform upstream gradient g_loss (mixed signs, three decades over the frames, one whole sequence and one frame of every
     sequence zero) -- under the constant 1 / (B N 9) a g_loss read per row, per sequence or without its sign is the same gradient;
  B. the regimes of the split reductions (pd_tr_chunks: min(16, ceil(M / 256)) chunks of a multiple of 32 rows): an odd M with a ragged
     last chunk, chunks of more than 256 rows under the 16-chunk cap, and the time embedding's weight gradients, which reduce over B,
     in two chunks;
  C. the attention backward with a sharp softmax (median largest probability >= 0.8, asserted on float64 before the engine runs), so
     that dQ and dK are a large part of in_proj's gradient, and at the head dims 12 and 68 and the frame counts 2, 4, 33, 63, 64;
  D. the limits of the trainer's configuration family (tr_shape_check) and its two head-dim refusals;
  E. one trainer reused for batches of changing shape, so that its stash still holds a larger batch's rows: bitwise the gradients of a
     fresh trainer of exactly that shape -- the header's contract -- directly and through the drop-in's ``engine_grad``;
  F. ``want`` subsets, bitwise against the full backward.
Bounds come from the float32 helper (4 x own, tests/train_checks.py) or are exact equalities between two engine runs that the header
declares bitwise equal, or exact zeros that float64 produces as well; no figure of the engine's own output enters a bound.  Every
figure is printed before it is asserted; profiles/train_grad_parity.txt records them."""
import pytest
import torch

from denoiser_cfgs import Cfg, build_dropin
from oracle import pd_oracle as O
import train_checks as TC
from posediffusion_amd import host, synth
from posediffusion_amd.schedule import diffusion_buffers
from posediffusion_amd.train import PoseTrainer, shape_from_modules
from test_gpu_train_grad import DEV, MARGIN, NONDEFAULT, RECORDED_MARGIN, _Net, _check_case, _engine_pass, _inputs, _inputs_for
from test_gpu_train_grad import default_net, small_net      # noqa: F401  (module-scoped fixtures: this module gets its own instances)

pytestmark = pytest.mark.gpu
ND = NONDEFAULT                                              # Cfg(96, 4, 200, 2, 50, 40, True, False), build_dropin(ND, seed=31)


def test_margins_are_the_rule():
    assert MARGIN == 4.0 and all(v <= 16.0 for v in RECORDED_MARGIN.values())


def _net_of(cfg, seed, qk_factor=1.0):
    den = build_dropin(cfg, seed)
    if qk_factor != 1.0:
        with torch.no_grad():
            for layer in den._trunk.layers:                  # rows [0, 2 d) of in_proj_weight: W_q and W_k, so every score is qk_factor^2 larger
                layer.self_attn.in_proj_weight[:2 * cfg.d] *= qk_factor
    return _Net(den)


# ------------------------------------------------------------------------------------------------ A. non-uniform upstream gradient
@pytest.mark.parametrize("shape,objective,loss_type", [((9, 15), "pred_noise", "l1"), ((9, 15), "pred_noise", "l2"), ((3, 7), "pred_x0", "l1")],
                         ids=["b9n15-l1", "b9n15-l2", "b3n7-x0-l1"])
def test_non_uniform_g_loss(small_net, shape, objective, loss_type):
    g_loss = TC.draw_g_loss(*shape)
    grads = _check_case(small_net, _inputs_for(small_net, *shape), objective, loss_type, label=f"A {ND.name} {shape} {objective} {loss_type}",
                        g_loss=g_loss)
    assert grads["z"][0].abs().max().item() == 0.0 and grads["z"][:, 1].abs().max().item() > 0.0     # a zero FRAME still gets dz through attention


def test_non_uniform_g_loss_default_net(default_net):
    grads = _check_case(default_net, _inputs_for(default_net, 3, 5), "pred_noise", "l1", label="A default (3, 5) pred_noise l1",
                        g_loss=TC.draw_g_loss(3, 5))
    assert grads["z"][0].abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------------ B. reduction-chunk regimes
# pd_tr_chunks(M): n = min(16, ceil(M / 256)); rows = ceil(M / n) rounded up to a multiple of 32; chunks = ceil(M / rows).  The time
# embedding's two weight gradients reduce over B with the same function.
CHUNK_SHAPES = [
    (257, 1),    # M 257: n 2, rows 160 -> 2 chunks, the last of 97 rows (odd M); over B = 257 the same split; N = 1: q, k gradients exactly 0
    (9, 57),     # M 513: n 3, rows 192 -> 3 chunks, the last of 129 rows; B = 9: one chunk
    (300, 2),    # M 600: n 3, rows 224 -> 3 chunks, the last of 152 rows; over B = 300: 2 chunks of 160, the last of 140; pd_tr_tsum_kernel at N = 2
    (60, 64),    # M 3840: n 15, rows 256 -> 15 chunks of exactly 256 rows, no tail
    (66, 64),    # M 4224: n capped at 16, rows 264 -> 288 -> 15 chunks, the last of 192 rows
]


def _chunks(M):                                              # the formula above, for the comments' figures only
    n = min(16, -(-M // 256))
    rows = -(-(-(-M // n)) // 32) * 32
    return -(-M // rows), rows, M - (-(-M // rows) - 1) * rows


def test_chunk_figures_of_the_cases():
    assert [_chunks(b * n) for b, n in CHUNK_SHAPES] == [(2, 160, 97), (3, 192, 129), (3, 224, 152), (15, 256, 256), (15, 288, 192)]
    assert _chunks(257)[:2] == (2, 160) and _chunks(300) == (2, 160, 140) and _chunks(100)[0] == 1


@pytest.mark.parametrize("shape", CHUNK_SHAPES, ids=[f"b{b}n{n}" for b, n in CHUNK_SHAPES])
def test_reduction_chunk_regimes(small_net, shape):
    inp = _inputs_for(small_net, *shape)
    if shape[0] > 100:
        t = inp["t"].tolist()
        assert 0 in t and 99 in t and len(set(t)) < shape[0]
    _check_case(small_net, inp, "pred_noise", "l1", label=f"B {ND.name} {shape}")


# ------------------------------------------------------------------------------------------------ C. attention backward where it matters
@pytest.fixture(scope="module")
def sharp_net():
    n = _net_of(ND, 31, qk_factor=4.0)
    yield n
    n.close()


@pytest.mark.parametrize("shape", [(9, 15), (2, 64)], ids=["b9n15", "b2n64"])
def test_sharp_softmax(sharp_net, shape):
    inp = _inputs_for(sharp_net, *shape)
    sd64 = {k: v.double() for k, v in sharp_net.sd.items()}
    x_t = TC.q_sample(inp["x_start"].double(), inp["noise"].double(), inp["t"], O.diffusion_tables(dtype=torch.float64))
    with torch.no_grad():
        pmax = TC.denoiser_forward(sd64, sharp_net.net, x_t, inp["t"], inp["z"].double())[1]["pmax"]
    medians = [p.flatten().median().item() for p in pmax]
    print(f"C sharp {shape}: median over softmax rows of the largest probability, per layer: {[f'{m:.3f}' for m in medians]} (uniform {1 / shape[1]:.3f})")
    assert all(m >= 0.8 for m in medians), medians           # float64 alone, before the engine runs
    _check_case(sharp_net, inp, "pred_noise", "l1", label=f"C sharp {ND.name} {shape}")


HEAD_DIM_CASES = [
    (Cfg(96, 8, 96, 2, 35, 24, True, True), 49, [(3, 2), (3, 4), (2, 33), (2, 63), (2, 64)]),      # head dim 12: three float4 per row; Kf = 353
    (Cfg(544, 8, 128, 1, 8, 64, True, False), 50, [(2, 64), (3, 5)]),                              # head dim 68: output slot 1 of a lane partly used
]


@pytest.mark.parametrize("cfg,seed,shapes", HEAD_DIM_CASES, ids=[c.name for c, _, _ in HEAD_DIM_CASES])
def test_head_dim_and_frame_count_edges(cfg, seed, shapes):
    net = _net_of(cfg, seed)
    try:
        for shape in shapes:
            _check_case(net, _inputs_for(net, *shape), "pred_noise", "l1", label=f"C {cfg.name} {shape}")
    finally:
        net.close()


# ------------------------------------------------------------------------------------------------ D. the family's limits
LIMIT_CFGS = [
    Cfg(32, 4, 64, 2, 16, 32, True, True),                   # smallest d, head dim 8
    Cfg(160, 8, 65, 1, 34, 65, True, True),                  # ff and hidden one past 64; Kf = 352
    Cfg(128, 1, 64, 1, 16, 32, True, True),                  # one head of 128
    Cfg(2048, 16, 64, 1, 16, 32, True, False),               # largest d, head dim 128
    Cfg(64, 2, 8192, 1, 16, 32, True, True),                 # largest ff
    Cfg(64, 4, 1, 2, 1, 20, True, True),                     # ff = z = 1
    Cfg(64, 4, 1, 2, 1, 1, True, True),                      # hidden = 1: the tail's LayerNorm output is its beta
    Cfg(64, 4, 128, 1, 4096, 1024, True, True),              # largest z and hidden
    Cfg(64, 8, 128, 16, 32, 64, True, False),                # 16 layers
]


@pytest.mark.parametrize("i", range(len(LIMIT_CFGS)), ids=[c.name for c in LIMIT_CFGS])
def test_family_limits(i):
    cfg = LIMIT_CFGS[i]
    net = _net_of(cfg, 40 + i)
    try:
        grads = _check_case(net, _inputs_for(net, 3, 7), "pred_noise", "l1", label=f"D {cfg.name} (3, 7)")
        if cfg.hidden == 1:
            # LayerNorm of one value is its beta: nothing upstream of _last.1.bias reaches the loss.  float64's gradient of 33 of the 36
            # parameter tensors and of z is identically zero (all but _last.1.bias, _last.3.weight, _last.3.bias); _check_case has
            # asserted that the engine's are exactly zero wherever float64's are
            zero = sorted(n for n, g in grads.items() if g.abs().max().item() == 0.0)
            print(f"D {cfg.name}: {len(zero)} of {len(grads)} gradients are exactly zero")
            assert len(zero) == 34 and "z" in zero and not {"_last.1.bias", "_last.3.weight", "_last.3.bias"} & set(zero)
    finally:
        net.close()


def test_head_dim_refusals_launch_nothing_and_leave_the_library_usable(small_net):
    bufs = diffusion_buffers()
    for d, heads in [(96, 16), (32, 8)]:                     # head dim 6 (no multiple of 4) and 4 (below 8)
        with pytest.raises(RuntimeError, match=r"code -2.*multiple of 4, at least 8"):
            PoseTrainer(dict(small_net.shape, d_model=d, nhead=heads), bufs, 3, 7, device=torch.device(DEV))
    inp = _inputs(3, 7, ND.z)
    after = PoseTrainer(dict(small_net.shape), bufs, 3, 7, device=torch.device(DEV))
    try:
        _, _, a = _engine_pass(after, small_net, inp, "l1")
    finally:
        after.close()
    _, _, b = _engine_pass(small_net.trainer("pred_noise", 3, 7), small_net, inp, "l1")
    assert all(torch.isfinite(a[n]).all() and torch.equal(a[n], b[n]) for n in b)


# ------------------------------------------------------------------------------------------------ E. a reused trainer
def _assert_bitwise(got, want, what):
    (out_g, relu_g, grads_g), (out_w, relu_w, grads_w) = got, want
    assert set(out_g) == set(out_w) and set(grads_g) == set(grads_w)
    for k in out_w:
        assert torch.equal(out_g[k], out_w[k]), (what, k)
    for l, (a, b) in enumerate(zip(relu_g, relu_w)):
        assert torch.equal(a, b), (what, "relu", l)
    for n in grads_w:
        assert torch.equal(grads_g[n], grads_w[n]), (what, n)


def test_reused_trainer_is_bitwise_a_fresh_one(small_net):
    """One trainer of capacity (66, 64) over batches of changing shape: every step's stash is written over rows a larger batch left
    there, and (step 4, a forward without its backward) over a stash that was never consumed."""
    bufs, shape = diffusion_buffers(), dict(small_net.shape, objective="pred_noise")
    steps = [((66, 64), "l1"), ((3, 7), "l2"), ((9, 57), "l1"), None, ((1, 1), "l1"), ((40, 20), "l2"), ((3, 7), "l1")]
    big = PoseTrainer(shape, bufs, 66, 64, device=torch.device(DEV))
    try:
        for step in steps:
            if step is None:                                 # a forward that is never followed by a backward: the stash is overwritten, not consumed
                inp = _inputs(40, 20, ND.z)
                big.forward(small_net.gpu, inp["x_start"], inp["z"], inp["t"], inp["noise"], "l2")
                continue
            (B, N), loss_type = step
            inp = _inputs(B, N, ND.z)
            got = _engine_pass(big, small_net, inp, loss_type)
            fresh = PoseTrainer(shape, bufs, B, N, device=torch.device(DEV))
            try:
                want = _engine_pass(fresh, small_net, inp, loss_type)
            finally:
                fresh.close()
            _assert_bitwise(got, want, f"({B}, {N}) {loss_type}")
            assert all(torch.isfinite(g).all() for g in got[2].values())
    finally:
        big.close()


def test_reused_trainer_through_the_dropin():
    models = synth._dropin()
    diff = models.GaussianDiffusion(beta_schedule="custom")
    diff.model = build_dropin(ND, seed=31)
    diff = diff.to(DEV).eval()
    diff.engine_grad = True
    bufs = {n: b for n, b in diff.named_buffers(recurse=False)}
    B, first = 4, None
    for N in (12, 5, 9):
        inp = {k: v.to(DEV) for k, v in _inputs(B, N, ND.z).items()}
        diff.model.zero_grad(set_to_none=True)
        z = inp["z"].clone().requires_grad_()
        r = diff.p_losses(inp["x_start"], inp["t"], z=z, noise=inp["noise"])
        tr = host.get_trainer(diff.model, diff, B, N)
        first = first or tr
        assert tr is first and (tr.max_B, tr.max_N) == (B, 12)
        r["loss"].mean().backward()
        leaf = r["loss"].detach().clone().requires_grad_()   # the g_loss autograd hands the engine for .mean(), whatever its last bit
        leaf.mean().backward()
        params = {n: p.detach() for n, p in diff.model.named_parameters()}
        fresh = PoseTrainer(shape_from_modules(diff.model, diff), bufs, B, N, device=torch.device(DEV))
        try:
            out = fresh.forward(params, inp["x_start"], inp["z"], inp["t"], inp["noise"], diff.loss_type)
            want = fresh.backward(params, leaf.grad)
            torch.cuda.synchronize()
        finally:
            fresh.close()
        assert torch.equal(r["loss"].detach(), out["loss"]) and torch.equal(r["x_0_pred"], out["x_0_pred"]), N
        assert torch.equal(z.grad, want["z"]), (N, "z")
        for n, p in diff.model.named_parameters():
            assert p.grad is not None and torch.equal(p.grad, want[n]), (N, n)
    first.close()
    diff.model.__dict__.pop("_pd_trainer_cache", None)


# ------------------------------------------------------------------------------------------------ F. want subsets
def test_want_subsets_are_bitwise_the_full_backward(small_net):
    inp = _inputs(3, 7, ND.z)
    tr = small_net.trainer("pred_noise", 3, 7)
    _, _, full = _engine_pass(tr, small_net, inp, "l1")
    names = list(full)
    assert len(names) == 37 and "z" in names
    subsets = {
        "no in_proj_weight, no linear1.weight": [n for n in names if not n.endswith(("in_proj_weight", "linear1.weight"))],   # neither LayerNorm recompute
        "biases and LayerNorm tensors": [n for n in names if n.endswith("bias") or "norm" in n or n.startswith("_last.1")],
        "z only": ["z"],                                                                                                       # no time chain
        "time_embed.linear.0 only": ["time_embed.linear.0.weight", "time_embed.linear.0.bias"],                                # the time chain without time_w2
        "nothing": [],
    }
    assert len(subsets["no in_proj_weight, no linear1.weight"]) == 37 - 4 and "z" not in subsets["biases and LayerNorm tensors"]
    for what, sub in subsets.items():
        _, _, part = _engine_pass(tr, small_net, inp, "l1", want=sub)
        assert set(part) == set(sub), what
        for n in sub:
            assert torch.equal(part[n], full[n]), (what, n)
    _, _, again = _engine_pass(tr, small_net, inp, "l1")     # usable after the empty backward
    assert all(torch.equal(again[n], full[n]) for n in full)
