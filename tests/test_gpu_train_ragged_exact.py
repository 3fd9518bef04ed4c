"""GPU (-m gpu): the exact equalities the contract of pd_trainer_set_frame_counts states (include/pd_engine_train.h), between engine runs
that the header declares bitwise equal -- no tolerance anywhere except E6, which is the 4 x own rule of tests/test_gpu_train_ragged.py:

  E1 all counts = N: every output, stashed activation and gradient is bitwise the call without counts, with and without dropout, at
     (3, 7) and (2, 64) (counts force the key-tiled attention there, which gives the short kernels' bits) and at (3, 130);
  E2 slot b versus sequence b alone: loss, x_0_pred, x_t, model_out and dz of the slot's valid rows are bitwise those of the sequence
     run alone at N = n_frames[b] with the slot's t, inputs and g_loss rows;
  E3 padding content: NaN and 1e30 in the padding rows of x_start, noise, z and g_loss change no bit; through
     ``PoseDiffusionModel(image, gt_cameras=, training=True, n_frames=)`` with both ``engine_grad`` opt-ins, other images and cameras in
     the padding frames change no bit of any ``.grad``;
  E4 stale scratch: after a larger uniform batch on the same trainer the result is bitwise a fresh trainer's;
  E5 pending counts: ``set_frame_counts(None)`` or other counts between forward and backward change nothing;
  E6 the drop-in: ``GaussianDiffusion.p_losses(..., n_frames=)`` with ``engine_grad``, scaled ``loss.sum() / (9 sum(n))``, fills ``.grad``
     within 4 x own of the yardstick; under ``torch.no_grad()`` the same loss bits and no pending stash;
  E7 refusals (B mismatch, a count of 0, a count above N, N above the frame limit with counts set) leave a usable trainer."""
import numpy as np
import pytest
import torch

from denoiser_cfgs import build_dropin
from oracle import pd_oracle as O
import train_checks as TC
import train_ragged_checks as TR
from posediffusion_amd import host, synth
from posediffusion_amd.schedule import diffusion_buffers
from posediffusion_amd.train import PoseTrainer
from test_gpu_train_grad import DEV, MARGIN, NONDEFAULT, RECORDED_MARGIN, _inputs
from test_gpu_train_grad import small_net                   # noqa: F401  (module-scoped fixture: this module gets its own instance)
from test_gpu_train_ragged import DROP, engine_pass

pytestmark = pytest.mark.gpu
ND = NONDEFAULT
R1, R2 = ((3, 7), (7, 1, 4)), ((2, 64), (64, 33))


def _g_loss(B, N, seed=0):
    """mixed signs, no zero row: every slot and every frame has an upstream gradient"""
    g = torch.Generator().manual_seed(4400 + 100 * B + N + seed)
    return (torch.randn(B, N, 9, generator=g) + 0.25) / (B * N * 9)


def _assert_bitwise(got, want, what, rows=None):
    (out_g, relu_g, grads_g), (out_w, relu_w, grads_w) = got, want
    assert set(out_g) == set(out_w) and set(grads_g) == set(grads_w)
    for k in out_w:
        assert torch.equal(out_g[k], out_w[k]), (what, k)
    for l, (a, b) in enumerate(zip(relu_g, relu_w)):
        a, b = (a, b) if rows is None else (a[rows], b[rows])
        assert torch.equal(a, b), (what, "relu", l)
    for n in grads_w:
        assert torch.isfinite(grads_g[n]).all() and torch.equal(grads_g[n], grads_w[n]), (what, n)


def _fresh(net, B, N, max_frames=64):
    return PoseTrainer(dict(net.shape, objective="pred_noise"), diffusion_buffers(), B, N, device=torch.device(DEV), max_frames=max_frames)


# ------------------------------------------------------------------------------------------------ E1
@pytest.mark.parametrize("drop", [None, DROP], ids=["plain", "dropout"])
@pytest.mark.parametrize("B,N", [(3, 7), (2, 64), (3, 130)], ids=["b3n7", "b2n64", "b3n130"])
def test_e1_all_counts_equal_to_n_is_the_uniform_call(small_net, B, N, drop):
    inp, g = _inputs(B, N, ND.z), _g_loss(B, N)
    tr = _fresh(small_net, B, N, max_frames=256)
    try:
        assert tr.get_option(2) == 0                         # PD_TR_OPT_LONG_ATTN at its default: (3, 7) and (2, 64) run the short kernels
        want = engine_pass(tr, small_net, inp, None, "l1", g_loss=g, drop=drop)
        got = engine_pass(tr, small_net, inp, (N,) * B, "l1", g_loss=g, drop=drop)
    finally:
        tr.close()
    _assert_bitwise(got, want, f"({B}, {N}) all counts = N")
    assert any(v.abs().max() > 0 for v in want[2].values())


# ------------------------------------------------------------------------------------------------ E2
@pytest.mark.parametrize("shape,counts", [R1, R2], ids=["r1", "r2"])
@pytest.mark.parametrize("objective,loss_type", [("pred_noise", "l1"), ("pred_x0", "l2")])
def test_e2_a_slot_is_bitwise_its_sequence_alone(small_net, shape, counts, objective, loss_type):
    (B, N), g = shape, _g_loss(*shape)
    inp = _inputs(B, N, ND.z)
    tr = small_net.trainer(objective, B, N)
    out, _, grads = engine_pass(tr, small_net, inp, counts, loss_type, g_loss=g, want=["z"])
    for b, n in enumerate(counts):
        alone = small_net.trainer(objective, 1, n)
        o1, _, g1 = engine_pass(alone, small_net, TR.slice_sequence(inp, b, n), None, loss_type, g_loss=g[b:b + 1, :n], want=["z"])
        for k in ("loss", "x_0_pred", "x_t", "model_out"):
            assert torch.equal(out[k][b:b + 1, :n], o1[k]), (b, n, k)
        assert torch.equal(grads["z"][b:b + 1, :n], g1["z"]), (b, n, "dz")
        assert g1["z"].abs().max().item() > 0.0


# ------------------------------------------------------------------------------------------------ E3
@pytest.mark.parametrize("fill", [float("nan"), 1e30], ids=["nan", "1e30"])
@pytest.mark.parametrize("drop", [None, DROP], ids=["plain", "dropout"])
def test_e3_padding_rows_of_the_inputs_are_never_read(small_net, fill, drop):
    (B, N), counts = R1
    valid = TR.valid_rows(counts, N)[..., None]
    inp, g = _inputs(B, N, ND.z), _g_loss(B, N)
    zeroed = {k: (torch.where(valid, v, torch.zeros(())) if k != "t" else v) for k, v in inp.items()}
    poisoned = {k: (torch.where(valid, v, torch.full((), fill)) if k != "t" else v) for k, v in inp.items()}
    tr = small_net.trainer("pred_noise", B, N)
    want = engine_pass(tr, small_net, zeroed, counts, "l1", g_loss=torch.where(valid, g, torch.zeros(())), drop=drop)
    got = engine_pass(tr, small_net, poisoned, counts, "l1", g_loss=torch.where(valid, g, torch.full((), fill)), drop=drop)
    _assert_bitwise(got, want, f"padding = {fill}")
    assert all(torch.isfinite(r).all() for r in got[1]), "every stashed activation of a padding row is finite"


def test_e3_pose_diffusion_model_ignores_padding_frames():
    from test_gpu_vit_train import _model
    model = _model()
    B, N, counts = 2, 3, (3, 1)
    ext, diff = model.image_feature_extractor, model.diffuser
    ext.engine_grad = diff.engine_grad = True
    images = torch.rand(B, N, 3, 32, 32, generator=torch.Generator().manual_seed(12)).to(DEV)
    other = images.clone()
    other[1, 1:] = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(13)).to(DEV)
    encs = [np.concatenate([synth.make_cameras(N, seed=700 + s + b) for b in range(B)]) for s in (0, 50)]
    encs[1][:N + 1] = encs[0][:N + 1]                        # the cameras of the valid frames stay, the two padding frames get others
    assert not np.array_equal(encs[0][N + 1:], encs[1][N + 1:])

    def cams(enc):
        from posediffusion_amd.compat import PerspectiveCameras
        c = O.pose_encoding_to_camera(torch.from_numpy(enc).float())
        return PerspectiveCameras(focal_length=c["focal_length"].to(DEV), R=c["R"].to(DEV), T=c["T"].to(DEV), device=torch.device(DEV))

    runs = []
    for img, enc in ((images, encs[0]), (other, encs[1])):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1)
        out = model(image=img, gt_cameras=cams(enc), training=True, n_frames=counts)
        assert out["loss"].requires_grad and out["loss"].shape == (B, N, 9) and (out["loss"][1, 1:] == 0).all()
        (out["loss"].sum() / (9 * sum(counts))).backward()
        runs.append({f"{fam}.{n}": p.grad.clone() for fam, mod in (("denoiser", diff.model), ("backbone", ext._net)) for n, p in mod.named_parameters()})
    for n, g in runs[0].items():
        assert torch.isfinite(g).all() and g.abs().max() > 0, n
        assert torch.equal(g, runs[1][n]), n


# ------------------------------------------------------------------------------------------------ E4
def test_e4_a_larger_uniform_batch_leaves_nothing_behind(small_net):
    (B, N), counts = R1
    inp, g = _inputs(B, N, ND.z), _g_loss(B, N)
    big, fresh = _fresh(small_net, 4, 20), _fresh(small_net, B, N)
    try:
        engine_pass(big, small_net, _inputs(4, 20, ND.z), None, "l1")
        got = engine_pass(big, small_net, inp, counts, "l1", g_loss=g)
        want = engine_pass(fresh, small_net, inp, counts, "l1", g_loss=g)
    finally:
        big.close()
        fresh.close()
    _assert_bitwise(got, want, "after (4, 20)", rows=TR.valid_rows(counts, N).reshape(-1))


# ------------------------------------------------------------------------------------------------ E5
def test_e5_the_counts_of_a_forward_belong_to_its_stash(small_net):
    (B, N), counts = R1
    inp, g = _inputs(B, N, ND.z), _g_loss(B, N).to(DEV)
    tr = small_net.trainer("pred_noise", B, N)
    want = engine_pass(tr, small_net, inp, counts, "l1", g_loss=g)
    for between in (None, (2, 7, 6)):
        tr.forward(small_net.gpu, inp["x_start"], inp["z"], inp["t"], inp["noise"], "l1", n_frames=counts)
        tr.set_frame_counts(between)
        grads = {k: v.cpu() for k, v in tr.backward(small_net.gpu, g).items()}
        tr.set_frame_counts(None)
        for n in grads:
            assert torch.equal(grads[n], want[2][n]), (between, n)


# ------------------------------------------------------------------------------------------------ E6
def test_e6_dropin_p_losses_with_n_frames():
    models = synth._dropin()
    diff = models.GaussianDiffusion(beta_schedule="custom")
    diff.model = build_dropin(ND, seed=31)
    diff = diff.to(DEV).eval()
    diff.engine_grad = True
    (B, N), counts = R1
    inp = _inputs(B, N, ND.z)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    z = dev["z"].clone().requires_grad_()
    r = diff.p_losses(dev["x_start"], dev["t"], z=z, noise=dev["noise"], n_frames=counts)
    assert sorted(r) == ["loss", "noise", "t", "x_0_pred", "x_t"] and r["loss"].requires_grad
    tr = host.get_trainer(diff.model, diff, B, N)
    masks = [tr.debug_relu(l).cpu() > 0 for l in range(ND.layers + 1)]
    (r["loss"].sum() / (9 * sum(counts))).backward()
    sd = {k: v.detach().cpu().clone() for k, v in diff.model.state_dict().items()}
    net = TC.Net.of_cfg(ND)
    own64 = TR.loss_and_grads(sd, net, inp, counts, diff.objective, diff.loss_type, want=[])
    forced = dict(masks=masks, signs=own64["signs"])
    r64 = TR.loss_and_grads(sd, net, inp, counts, diff.objective, diff.loss_type, **forced)
    r32 = TR.loss_and_grads(sd, net, inp, counts, diff.objective, diff.loss_type, dtype=torch.float32, **forced)
    got = {n: p.grad for n, p in diff.model.named_parameters()}
    got["z"] = z.grad
    misses = []
    for n, g in got.items():
        assert g is not None and torch.isfinite(g).all(), n
        e, own = TC.grad_dist(g, r64["grads"][n]), TC.grad_dist(r32["grads"][n], r64["grads"][n])
        print(f"E6 {n}: engine {e:.3e} own {own:.3e}")
        if e > RECORDED_MARGIN.get(n, MARGIN) * own:
            misses.append((n, e, own))
    assert not misses, misses
    valid = TR.valid_rows(counts, N)
    assert (z.grad.cpu()[~valid] == 0).all() and (r["loss"].detach().cpu()[~valid] == 0).all()
    with torch.no_grad():
        r2 = diff.p_losses(dev["x_start"], dev["t"], z=dev["z"], noise=dev["noise"], n_frames=counts)
    assert not r2["loss"].requires_grad and torch.equal(r2["loss"], r["loss"].detach()) and tr._pending is None
    assert host.get_trainer(diff.model, diff, B, N) is tr and "_pd_engine_cache" not in diff.model.__dict__      # the engine was never asked
    diff.engine_grad = False                                 # forward only through the trainer as well: the engine keeps refusing counts
    r3 = diff.p_losses(dev["x_start"], dev["t"], z=dev["z"], noise=dev["noise"], n_frames=counts)
    assert not r3["loss"].requires_grad and torch.equal(r3["loss"], r2["loss"]) and tr._pending is None
    tr.close()
    diff.model.__dict__.pop("_pd_trainer_cache", None)


# ------------------------------------------------------------------------------------------------ E7
def test_e7_refusals_leave_a_usable_trainer(small_net):
    (B, N), counts = R1
    inp = _inputs(B, N, ND.z)
    tr = _fresh(small_net, 4, 70)
    try:
        before = engine_pass(tr, small_net, inp, None, "l1")
        args = (small_net.gpu, inp["x_start"], inp["z"], inp["t"], inp["noise"], "l1")
        tr.set_frame_counts((7, 1))                          # the ABI's own refusals: counts for another B ...
        with pytest.raises(RuntimeError, match=r"code -1.*pd_train_forward: frame counts per sequence are set for B=2.*called with B=3"):
            tr.forward(*args)
        tr.set_frame_counts((7, 8, 4))                       # ... a count above N (admitted by the capacity, refused at the forward) ...
        with pytest.raises(RuntimeError, match=r"code -1.*n_frames\[1\]=8 .* exceeds N=7: every count must lie in \[1, N\]"):
            tr.forward(*args)
        with pytest.raises(RuntimeError, match=r"code -1.*n_frames\[1\]=0: every count must lie in \[1, N\]"):
            tr.set_frame_counts((7, 0, 4))                   # ... a count of 0 ...
        with pytest.raises(RuntimeError, match=r"code -1.*n_frames\[0\]=71"):
            tr.set_frame_counts((71, 1, 4))
        long = _inputs(B, 70, ND.z)
        tr.set_frame_counts((70, 1, 4))                      # ... and N above the frame limit while counts are set
        with pytest.raises(RuntimeError, match=r"code -2.*limit of 64 frames"):
            tr.forward(small_net.gpu, long["x_start"], long["z"], long["t"], long["noise"], "l1")
        with pytest.raises(RuntimeError, match=r"code -4.*no forward is pending"):
            tr.backward(small_net.gpu, torch.zeros(B, N, 9, device=DEV))
        tr.set_frame_counts(None)
        for bad, msg in (((7, 1), "one frame count per sequence"), ((7, 0, 4), r"\[1, N\]"), ((7, 8, 4), r"\[1, N\]")):
            with pytest.raises(ValueError, match=msg):       # the keyword validates in Python, and leaves no counts behind
                tr.forward(*args, n_frames=bad)
        after = engine_pass(tr, small_net, inp, None, "l1")
        _assert_bitwise(after, before, "a uniform call after the refusals")
        ragged = engine_pass(tr, small_net, inp, counts, "l1")
        assert all(torch.isfinite(v).all() for v in ragged[2].values())
    finally:
        tr.close()
