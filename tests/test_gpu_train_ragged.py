"""GPU (-m gpu): sequences of different frame counts in one padded batch on the trainer -- pd_trainer_set_frame_counts
(include/pd_engine_train.h) through ``PoseTrainer.forward(..., n_frames=)`` -- against the float64 yardstick on the padded layout
(tests/train_ragged_checks.py, pinned by tests/test_train_ragged_checks_cpu.py).

The method is tests/test_gpu_train_grad.py's, teacher-forced: forward, the engine's ReLU masks and loss signs, backward, then
  * the MASK condition over the VALID rows (masks of padding rows are unconstrained): at most 1e-5 of the ReLU activations differ from
    float64's own, no loss sign differs, the stash is within 4 x own of float64's;
  * PARITY: loss, model_out, every parameter gradient, dz and every sub-block (train_checks.grad_blocks) within 4 x the float32
    helper's own distance from float64 with the same masks forced (16 x for ``time_embed.linear.0.weight``, RECORDED_MARGIN); exact
    zeros where float64's are zero;
  * padding rows of loss, x_0_pred, x_t, model_out and dz are exactly +0.
No figure of the engine's own output enters a bound.  Every figure is printed before it is asserted; profiles/train_ragged_parity.txt
records them.  The cases:
  R1 (3, 7) counts (7, 1, 4), pred_noise / l1 and pred_x0 / l2: a full slot beside short ones, a count of 1 (one key per softmax row);
  R2 (2, 64) counts (64, 33): the short / tiled boundary -- counts force the key-tiled family at N <= 64;
  R3 (3, 15) counts (15, 2, 9) under a sharp softmax (median largest probability >= 0.8 over valid rows and keys, asserted on float64
     before the engine runs): a padded key that leaks takes real mass;
  R4 the default net, (3, 5) counts (5, 2, 3) with TC.draw_g_loss: pivot on, non-uniform upstream gradient (non-zero at padding rows
     too -- they must not be read);
  R5 max_frames = 256: (3, 130) counts (130, 65, 64) -- the tile edges 64 | 65 and a last tile of 2 keys -- and (2, 256) counts (256, 1);
  R6 dropout p = 0.1 at all four sites: (3, 7) counts (7, 1, 4) and, with max_frames = 256, (2, 70) counts (70, 65); the masks come from
     the helper on the PADDED layout, so a mask row computed with the count instead of the stride fails for every head >= 1."""
import pytest
import torch

from denoiser_cfgs import build_dropin
from oracle import pd_oracle as O
import train_checks as TC
import train_dropout_checks as TD
import train_ragged_checks as TR
from posediffusion_amd.schedule import diffusion_buffers
from posediffusion_amd.train import PoseTrainer
from test_gpu_train_grad import DEV, MARGIN, NONDEFAULT, RECORDED_MARGIN, _Net, _inputs
from test_gpu_train_grad import default_net, small_net      # noqa: F401  (module-scoped fixtures: this module gets its own instances)

pytestmark = pytest.mark.gpu
ND = NONDEFAULT                                              # Cfg(96, 4, 200, 2, 50, 40, True, False), build_dropin(ND, seed=31)
DROP = (0.1, TD.ALL, 23, 2)                                  # p, sites, seed, step of R6


def _drop_kw(drop):
    return {} if drop is None else dict(p=drop[0], sites=drop[1], seed=drop[2], step=drop[3])


def _pre64(net, inp, counts, drop):
    """float64's own ReLU inputs on the padded layout, no grad."""
    with torch.no_grad():
        sd = {k: v.double() for k, v in net.sd.items()}
        valid = TR.valid_rows(counts, inp["x_start"].shape[1])
        x0, nz, z = (TR.zero_padding(inp[k].double(), valid) for k in ("x_start", "noise", "z"))
        x_t = TC.q_sample(x0, nz, inp["t"], O.diffusion_tables(dtype=torch.float64))
        sites, d3 = (0, (0.0, 0, 0)) if drop is None else (drop[1], (drop[0], drop[2], drop[3]))
        return TR.denoiser_forward(sd, net.net, x_t, inp["t"], z, valid, sites, d3)[1]["pre"], valid


def inputs_for(net, B, N, counts, drop=None):
    """test_gpu_train_grad._inputs_for over the valid rows: where the case admits no differing mask (fewer than 1e5 activations), the
    first draw for which float64 has no activation of a VALID row inside the band u sqrt(d_model) x the layer's largest."""
    zdim, d = net.shape["z_dim"], net.shape["d_model"]
    total = sum(counts) * (net.net.layers * net.shape["dim_ff"] + net.shape["mlp_hidden"])
    for seed in range(16):
        inp = _inputs(B, N, zdim, seed)
        if 1e-5 * total >= 1.0:
            return inp
        pre, valid = _pre64(net, inp, counts, drop)
        if all(a[valid].abs().min().item() > 2.0 ** -24 * d ** 0.5 * a[valid].max().item() for a in pre):
            return inp
    raise AssertionError("no well-posed draw among 16 seeds")


def engine_pass(tr, net, inp, counts, loss_type, g_loss=None, drop=None, want=None):
    """forward with ``n_frames=counts`` (None: a uniform call), the stashed ReLU values, backward with ``g_loss`` (None: the mean over
    real frames, 1 / (9 sum(counts)) on valid rows) -> (outputs, relu, grads) on the CPU."""
    B, N, _ = inp["x_start"].shape
    kw = {} if drop is None else dict(dropout_p=drop[0], dropout_sites=drop[1], seed=drop[2], step=drop[3])
    out = tr.forward(net.gpu, inp["x_start"], inp["z"], inp["t"], inp["noise"], loss_type, n_frames=counts, **kw)
    tr.check_async()
    relu = [tr.debug_relu(l).cpu() for l in range(net.net.layers + 1)]
    if g_loss is None:
        g_loss = TR.default_g_loss(counts if counts is not None else (N,) * B, N, torch.float32)
    grads = tr.backward(net.gpu, g_loss.to(DEV), want)
    return {k: v.cpu() for k, v in out.items()}, relu, {k: v.cpu() for k, v in grads.items()}


def assert_padding_is_plus_zero(out, grads, valid, label):
    for k, v in list(out.items()) + [("dz", grads["z"])]:
        pad = v[~valid]
        assert (pad == 0).all() and not torch.signbit(pad).any(), (label, k, "padding rows must be +0")


def check_ragged(net, inp, counts, objective, loss_type, tr=None, label="", g_loss=None, drop=None):
    B, N, _ = inp["x_start"].shape
    tr = tr or net.trainer(objective, B, N)
    out, relu, grads = engine_pass(tr, net, inp, counts, loss_type, g_loss=g_loss, drop=drop)
    valid = TR.valid_rows(counts, N)
    vflat = valid.reshape(-1)
    assert_padding_is_plus_zero(out, grads, valid, label)
    target = inp["noise"] if objective == "pred_noise" else inp["x_start"]
    masks_e = [r > 0 for r in relu]
    signs_e = torch.where(valid[..., None], torch.sign(out["model_out"] - target), torch.zeros(()))
    args, kw = (net.sd, net.net, inp, counts, objective, loss_type), dict(g_loss=g_loss, **_drop_kw(drop))
    own64 = TR.loss_and_grads(*args, want=[], **kw)
    r64 = TR.loss_and_grads(*args, masks=masks_e, signs=signs_e, **kw)
    r32 = TR.loss_and_grads(*args, masks=masks_e, signs=signs_e, dtype=torch.float32, **kw)
    total = sum(int(vflat.sum()) * m.shape[-1] for m in masks_e)
    ndiff, problems = 0, []
    fscale = TD.scale_of(drop[0]) if drop is not None and drop[1] & TD.FF else 1.0
    for l, (me, a64, a32, post) in enumerate(zip(masks_e, own64["pre"], r32["pre"], relu)):
        keep = torch.ones_like(me)
        if drop is not None and drop[1] & TD.FF and l < net.net.layers:                 # the FF site's mask, rows m = b N + i of the PADDED layout
            keep = torch.from_numpy(TD.keep_mask(B * N, me.shape[-1], l, 2, drop[2], drop[3], drop[0]))
        ks = keep.double() * (fscale if l < net.net.layers else 1.0)
        a64, a32 = a64.reshape(me.shape), a32.reshape(me.shape).double()
        want = (a64.clamp_min(0) * ks)[vflat]
        scale = max(want.abs().max().item(), 1e-300)
        own = ((a32.clamp_min(0) * ks)[vflat] - want).abs().max().item() / scale
        e = (post.double()[vflat] - want).abs().max().item() / scale
        differ = (me != ((a64 > 0) & keep))[vflat]
        ndiff += int(differ.sum())
        worst_flip = a64[vflat][differ].abs().max().item() / scale if differ.any() else 0.0
        print(f"{label} relu {l}: stash {e:.3e} own {own:.3e}; {int(differ.sum())} flips over valid rows, largest |a64| {worst_flip:.3e}")
        if e > MARGIN * own:
            problems.append(("stash", l, e, own))
        if worst_flip > MARGIN * own:
            problems.append(("flip magnitude", l, worst_flip, own))
    nsign = int((signs_e.double() != TR.zero_padding(own64["signs"], valid)).sum())
    print(f"{label} masks: {ndiff} of {total} valid-row activations differ from float64's own; loss signs differing: {nsign}")
    assert ndiff <= 1e-5 * total, (ndiff, total)
    assert nsign == 0
    for k in ("model_out", "loss", "x_t"):
        e, own = TC.grad_dist(out[k], r64[k]), TC.grad_dist(r32[k], r64[k])
        print(f"{label} {k}: engine {e:.3e} own {own:.3e}")
        if e > MARGIN * own:
            problems.append((k, e, own))
    worst, worst_block = (0.0, "", 0.0, 0.0), (0.0, "", 0.0, 0.0)
    d, zdim = net.shape["d_model"], net.shape["z_dim"]
    for n in list(net.sd) + ["z"]:
        g64, g = r64["grads"][n], grads[n]
        assert torch.isfinite(g).all(), n
        if g64.abs().max().item() == 0.0:
            assert g.abs().max().item() == 0.0, (n, "float64 gradient is identically zero")
            continue
        e, own = TC.grad_dist(g, g64), TC.grad_dist(r32["grads"][n], g64)
        if e / max(own, 1e-30) > worst[0]:
            worst = (e / max(own, 1e-30), n, e, own)
        if e > RECORDED_MARGIN.get(n, MARGIN) * own:
            print(f"{label} PARITY MISS {n}: engine {e:.3e} own {own:.3e} ({e / own:.2f} x)")
            problems.append(("parity", n, e, own))
        for bn, be, bown, zero in TC.block_dists(n, g, r32["grads"][n], g64, d, zdim):
            ratio = 0.0 if zero else be / max(bown, 1e-30)
            if not (n.endswith("in_proj_bias") and bn == "k") and ratio > worst_block[0]:
                worst_block = (ratio, f"{n}[{bn}]", be, bown)
        for bn, be, bown in TC.block_misses(n, g, r32["grads"][n], g64, d, zdim, MARGIN, RECORDED_MARGIN):
            print(f"{label} BLOCK MISS {bn}: engine {be:.3e} own {bown:.3e}")
            problems.append(("block", bn, be, bown))
    print(f"{label} parity: worst engine / own = {worst[0]:.2f} ({worst[1]}: engine {worst[2]:.3e}, own {worst[3]:.3e})")
    print(f"{label} blocks: worst engine / own = {worst_block[0]:.2f} ({worst_block[1]}: engine {worst_block[2]:.3e}, own {worst_block[3]:.3e})")
    assert (r64["grads"]["z"][~valid] == 0).all()            # float64's dz is zero at padding, so is the engine's (asserted above)
    assert not problems, problems
    return out, grads


def long_trainer(net, objective, B, N):
    return PoseTrainer(dict(net.shape, objective=objective), diffusion_buffers(), B, N, device=torch.device(DEV), max_frames=256)


# ------------------------------------------------------------------------------------------------ R1, R2
@pytest.mark.parametrize("objective,loss_type", [("pred_noise", "l1"), ("pred_x0", "l2")])
def test_r1_a_full_slot_beside_short_ones_and_a_count_of_one(small_net, objective, loss_type):
    counts = (7, 1, 4)
    check_ragged(small_net, inputs_for(small_net, 3, 7, counts), counts, objective, loss_type, label=f"R1 {ND.name} (3, 7) {counts} {objective} {loss_type}")


def test_r2_counts_force_the_tiled_family_at_64_frames(small_net):
    counts = (64, 33)
    check_ragged(small_net, inputs_for(small_net, 2, 64, counts), counts, "pred_noise", "l1", label=f"R2 {ND.name} (2, 64) {counts}")


# ------------------------------------------------------------------------------------------------ R3
def test_r3_sharp_softmax_a_leaking_padded_key_takes_real_mass():
    den = build_dropin(ND, 31)
    with torch.no_grad():
        for layer in den._trunk.layers:                      # rows [0, 2 d) of in_proj_weight: W_q and W_k, so every score is 16 x larger
            layer.self_attn.in_proj_weight[:2 * ND.d] *= 4.0
    net = _Net(den)
    try:
        counts = (15, 2, 9)
        inp = inputs_for(net, 3, 15, counts)
        pmax = TR.loss_and_grads(net.sd, net.net, inp, counts, "pred_noise", "l1", want=[])["pmax"]
        medians = [torch.cat([p[b, :, :n].flatten() for b, n in enumerate(counts)]).median().item() for p in pmax]
        print(f"R3 sharp {counts}: median over valid softmax rows of the largest probability over valid keys, per layer: {[f'{m:.3f}' for m in medians]}")
        assert all(m >= 0.8 for m in medians), medians       # float64 alone, before the engine runs
        check_ragged(net, inp, counts, "pred_noise", "l1", label=f"R3 sharp {ND.name} (3, 15) {counts}")
    finally:
        net.close()


# ------------------------------------------------------------------------------------------------ R4
def test_r4_default_net_pivot_and_non_uniform_g_loss(default_net):
    counts = (5, 2, 3)
    g_loss = TC.draw_g_loss(3, 5)
    assert g_loss[1, 2:].abs().max().item() > 0.0            # non-zero at padding rows: the engine must not read them
    _, grads = check_ragged(default_net, inputs_for(default_net, 3, 5, counts), counts, "pred_noise", "l1", label=f"R4 default (3, 5) {counts}", g_loss=g_loss)
    assert grads["z"][0].abs().max().item() == 0.0           # draw_g_loss: sequence 0 has no upstream gradient at all


# ------------------------------------------------------------------------------------------------ R5
@pytest.mark.parametrize("B,N,counts", [(3, 130, (130, 65, 64)), (2, 256, (256, 1))], ids=["b3n130", "b2n256"])
def test_r5_tile_edges_above_64_frames(small_net, B, N, counts):
    tr = long_trainer(small_net, "pred_noise", B, N)
    try:
        check_ragged(small_net, inputs_for(small_net, B, N, counts), counts, "pred_noise", "l1", tr=tr, label=f"R5 {ND.name} ({B}, {N}) {counts}")
    finally:
        tr.close()


# ------------------------------------------------------------------------------------------------ R6
@pytest.mark.parametrize("B,N,counts", [(3, 7, (7, 1, 4)), (2, 70, (70, 65))], ids=["b3n7", "b2n70"])
def test_r6_dropout_masks_of_the_padded_layout(small_net, B, N, counts):
    tr = long_trainer(small_net, "pred_noise", B, N)
    try:
        check_ragged(small_net, inputs_for(small_net, B, N, counts, DROP), counts, "pred_noise", "l1", tr=tr, drop=DROP,
                     label=f"R6 {ND.name} ({B}, {N}) {counts} p={DROP[0]}")
    finally:
        tr.close()
