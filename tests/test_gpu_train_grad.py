"""GPU (-m gpu): the training branch with gradients -- pd_train_forward / pd_train_backward (include/pd_engine_train.h) through
posediffusion_amd.train.PoseTrainer, and the drop-in opt-in ``GaussianDiffusion.engine_grad``.

The comparison is teacher-forced (tests/train_checks.py): the gradient is discontinuous at every ReLU threshold and at d = 0 under l1,
so every case
  1. runs pd_train_forward, 2. reads the engine's ReLU masks (pd_train_debug_relu) and loss signs, 3. runs pd_train_backward with
  g_loss = 1 / (B N 9) (= loss.mean()) unless the case brings its own, then checks
  * the MASK condition: the engine's masks differ from float64's own in at most 1e-5 of all activations, its loss signs in none; a
    differing activation has |a64| within the forward tolerance; the stashed post-ReLU values are within 4 x own of relu(a64), own being
    the float32 helper's distance on the same layer;
  * PARITY: per parameter tensor and for dz, max|g - g64| / max|g64| against the float64 helper with the engine's masks and signs forced
    is at most 4 x own, own being the float32 helper with the same forced masks; where the float64 gradient of a tensor (or, at N = 1,
    of the q and k rows of in_proj) is identically zero the engine's is exactly zero.  No blanket absolute tolerance.  The same 4 x own
    holds per sub-block (train_checks.grad_blocks: the q, k and v rows of in_proj_weight / in_proj_bias, the harmonic, x, t_emb, z and
    pivot columns of _first.weight), each against that block's own float64 maximum -- a tensor's maximum is its v rows, or its z
    columns, and an error in a smaller block would hide under it; the k rows of in_proj_bias are mathematically zero and are printed only.
Every figure is printed before it is asserted.  tests/test_gpu_train_grad_edges.py takes these helpers to the edge cases.

One tensor runs at the 16 x margin the rule allows once its distances and their cause are on record (profiles/train_grad_parity.txt):
``time_embed.linear.0.weight`` -- its gradient is da0^T [cos | sin](t f) and the yardstick's frequencies f are torch's fp32 ``exp`` on the
CPU, 3 of whose 128 values are one ulp from the correctly rounded ones the kernel uses; at t = 99 one ulp of f moves the angle by 6e-6.
Swapping the frequencies inside the float64 helper alone moves that gradient by 2.2e-6 (the engine's distance: 2.0e-6 - 2.1e-6, 1.5 x to
4.8 x own); every other tensor stays inside 4 x.

Inputs: a case of fewer than 1e5 activations admits NO differing mask, which is only meaningful if float64 itself has no activation
whose sign fp32 arithmetic cannot determine.  A pre-activation is a sum of d_model fp32 products; with unit roundoff u = 2^-24 its
accumulated rounding error is of the order u sqrt(d_model) times the layer's largest activation (5.8e-7 of it at d_model = 96), before any
error of its inputs.  `_inputs_for` draws such a case's inputs (seed 0, 1, ...) until float64's own activations all lie outside that
band -- a property of the yardstick and the number format alone, decided before the engine runs.  (The first draw at (9, 15) of the
non-default configuration has an activation at 3.9e-7 of its layer's largest; the engine's sign for it differed from float64's.)"""
import ctypes as C

import pytest
import torch

from denoiser_cfgs import Cfg, build_dropin
from oracle import pd_oracle as O
import train_checks as TC
from posediffusion_amd import _lib, host, synth
from posediffusion_amd.schedule import diffusion_buffers
from posediffusion_amd.train import PoseTrainer, shape_from_modules

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NONDEFAULT = Cfg(96, 4, 200, 2, 50, 40, True, False)        # head dim 24, no pivot: _first K = 367; K and N tails of every GEMM
MARGIN = 4.0
RECORDED_MARGIN = {"time_embed.linear.0.weight": 16.0}      # profiles/train_grad_parity.txt; never beyond 16; a sub-block's key is "tensor[block]"


def _inputs(B, N, zdim=384, seed=0):
    g = torch.Generator().manual_seed(9000 + 100 * B + N + seed)
    if B == 1:
        t = torch.tensor([0])
    elif (B, N) == (3, 5):
        t = torch.tensor([99, 0, 99])                       # a repeated timestep
    elif B > 100:                                           # more sequences than timesteps: repeats, with 0 and 99 forced in
        t = torch.randint(0, 100, (B,), generator=g)
        t[0], t[B - 1] = 0, 99
    else:
        t = torch.linspace(0, 99, B).round().long()[torch.randperm(B, generator=g)]      # distinct, with 0 and 99
        assert len(set(t.tolist())) == B and 0 in t.tolist() and 99 in t.tolist()
    return {"x_start": torch.randn(B, N, 9, generator=g), "noise": torch.randn(B, N, 9, generator=g),
            "z": synth.make_z(B, N, seed=9000 + B, z_dim=zdim), "t": t}


def _forward_pre(net, inp, dtype):
    """The helper's ReLU inputs (own masks) in ``dtype``, no grad."""
    with torch.no_grad():
        sd = {k: v.to(dtype) for k, v in net.sd.items()}
        x_t = TC.q_sample(inp["x_start"].to(dtype), inp["noise"].to(dtype), inp["t"], O.diffusion_tables(dtype=dtype))
        return TC.denoiser_forward(sd, net.net, x_t, inp["t"], inp["z"].to(dtype))[1]["pre"]


def _inputs_for(net, B, N):
    """`_inputs` of the case; where the case admits no differing mask (fewer than 1e5 activations), the first draw for which float64 has
    no activation inside the band u sqrt(d_model) x the layer's largest (see the module docstring)."""
    zdim, d = net.shape["z_dim"], net.shape["d_model"]
    total = B * N * (net.net.layers * net.shape["dim_ff"] + net.shape["mlp_hidden"])
    for seed in range(16):
        inp = _inputs(B, N, zdim, seed)
        if 1e-5 * total >= 1.0:
            return inp
        if all(a.abs().min().item() > 2.0 ** -24 * d ** 0.5 * a.max().item() for a in _forward_pre(net, inp, torch.float64)):
            return inp
    raise AssertionError("no well-posed draw among 16 seeds")


class _Net:
    """Weights of one configuration on both sides: float32 CPU state dict (the helper) and its copy on the GPU (the trainer's live tensors)."""

    def __init__(self, den, diffuser=None):
        self.sd = {k: v.detach().cpu().clone() for k, v in den.state_dict().items() if v.is_floating_point()}
        self.gpu = {k: v.to(DEV).contiguous() for k, v in self.sd.items()}
        self.shape = shape_from_modules(den, diffuser)
        self.net = TC.Net(self.shape["num_layers"], self.shape["nhead"], self.shape["pivot"])
        self._trainers = {}

    def trainer(self, objective, max_B, max_N):
        key = (objective, max_B, max_N)
        if key not in self._trainers:
            self._trainers[key] = PoseTrainer(dict(self.shape, objective=objective), diffusion_buffers(), max_B, max_N, device=torch.device(DEV))
        return self._trainers[key]

    def close(self):
        for t in self._trainers.values():
            t.close()


@pytest.fixture(scope="module")
def default_net(seeded_diffuser):
    n = _Net(seeded_diffuser.model)
    yield n
    n.close()


@pytest.fixture(scope="module")
def small_net():
    n = _Net(build_dropin(NONDEFAULT, seed=31))
    yield n
    n.close()


def _engine_pass(tr, net, inp, loss_type, want=None, g_loss=None):
    """forward, the stashed ReLU values, backward with ``g_loss`` ([B, N, 9]; None: 1 / (B N 9), i.e. loss.mean()) -> (outputs, relu, grads) on the CPU"""
    B, N, _ = inp["x_start"].shape
    out = tr.forward(net.gpu, inp["x_start"], inp["z"], inp["t"], inp["noise"], loss_type)
    tr.check_async()
    relu = [tr.debug_relu(l).cpu() for l in range(net.net.layers + 1)]
    g_loss = torch.full((B, N, 9), 1.0 / (B * N * 9), device=DEV) if g_loss is None else g_loss.to(DEV)
    grads = tr.backward(net.gpu, g_loss, want)
    return {k: v.cpu() for k, v in out.items()}, relu, {k: v.cpu() for k, v in grads.items()}


def _check_case(net, inp, objective, loss_type, tr=None, label="", g_loss=None):
    B, N, _ = inp["x_start"].shape
    tr = tr or net.trainer(objective, B, N)
    out, relu, grads = _engine_pass(tr, net, inp, loss_type, g_loss=g_loss)
    target = inp["noise"] if objective == "pred_noise" else inp["x_start"]
    masks_e = [r > 0 for r in relu]
    signs_e = torch.sign(out["model_out"] - target)
    # float64, its own masks: the mask condition
    own64 = TC.loss_and_grads(net.sd, net.net, inp, objective, loss_type, g_loss=g_loss, want=[])
    r64 = TC.loss_and_grads(net.sd, net.net, inp, objective, loss_type, g_loss=g_loss, masks=masks_e, signs=signs_e)
    r32 = TC.loss_and_grads(net.sd, net.net, inp, objective, loss_type, g_loss=g_loss, masks=masks_e, signs=signs_e, dtype=torch.float32)
    total = sum(m.numel() for m in masks_e)
    ndiff, problems = 0, []
    for l, (me, a64, a32, post) in enumerate(zip(masks_e, own64["pre"], r32["pre"], relu)):
        a64 = a64.reshape(me.shape)
        want = a64.clamp_min(0)
        scale = want.abs().max().item()
        own = (a32.reshape(me.shape).double().clamp_min(0) - want).abs().max().item() / scale
        e = (post.double() - want).abs().max().item() / scale
        differ = me != (a64 > 0)
        ndiff += int(differ.sum())
        worst_flip = a64[differ].abs().max().item() / scale if differ.any() else 0.0
        print(f"{label} relu {l}: stash {e:.3e} own {own:.3e}; {int(differ.sum())} flips, largest |a64| {worst_flip:.3e}")
        if e > MARGIN * own:
            problems.append(("stash", l, e, own))
        if worst_flip > MARGIN * own:
            problems.append(("flip magnitude", l, worst_flip, own))
    print(f"{label} masks: {ndiff} of {total} differ from float64's own; loss signs differing: {int((signs_e != own64['signs']).sum())}")
    assert ndiff <= 1e-5 * total, (ndiff, total)
    assert torch.equal(signs_e.double(), own64["signs"])
    # parity with the engine's masks and signs forced
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
        # the same rule per sub-block (q / k / v rows of in_proj, column groups of _first.weight), each against its own float64 maximum
        for bn, be, bown, zero in TC.block_dists(n, g, r32["grads"][n], g64, d, zdim):
            ratio = 0.0 if zero else be / max(bown, 1e-30)
            if n.endswith("in_proj_bias") and bn == "k":      # mathematically zero (train_checks.block_misses): left to the tensor-level bound
                kmax = [t[d:2 * d].abs().max().item() / g64.abs().max().item() for t in (g, r32["grads"][n], g64)]
                print(f"{label} {n}[k]: largest entry / the tensor's float64 maximum: engine {kmax[0]:.1e}, own {kmax[1]:.1e}, float64 {kmax[2]:.1e}")
            elif ratio > worst_block[0]:
                worst_block = (ratio, f"{n}[{bn}]", be, bown)
        for bn, be, bown in TC.block_misses(n, g, r32["grads"][n], g64, d, zdim, MARGIN, RECORDED_MARGIN):
            print(f"{label} BLOCK MISS {bn}: engine {be:.3e} own {bown:.3e}")
            problems.append(("block", bn, be, bown))
        if N == 1 and n.endswith(("in_proj_weight", "in_proj_bias")):
            assert g64[:2 * d].abs().max().item() == 0.0 and g[:2 * d].abs().max().item() == 0.0, n        # one key per softmax: q, k get nothing
    print(f"{label} parity: worst engine / own = {worst[0]:.2f} ({worst[1]}: engine {worst[2]:.3e}, own {worst[3]:.3e})")
    print(f"{label} blocks: worst engine / own = {worst_block[0]:.2f} ({worst_block[1]}: engine {worst_block[2]:.3e}, own {worst_block[3]:.3e})")
    if g_loss is not None:                                  # a sequence whose g_loss is all zero gets no gradient: attention does not mix sequences
        for b in range(B):
            if g_loss[b].abs().max().item() == 0.0:
                assert r64["grads"]["z"][b].abs().max().item() == 0.0 and grads["z"][b].abs().max().item() == 0.0, ("dz of sequence", b)
    assert not problems, problems
    return grads


DEFAULT_SHAPES = [(1, 1), (5, 13), (2, 64), (7, 19), (40, 20)]


@pytest.mark.parametrize("shape", DEFAULT_SHAPES, ids=[f"b{b}n{n}" for b, n in DEFAULT_SHAPES])
def test_default_cfg_gradients_vs_fp64(default_net, shape):
    _check_case(default_net, _inputs_for(default_net, *shape), "pred_noise", "l1", label=f"default {shape}")


@pytest.mark.parametrize("objective,loss_type", [("pred_noise", "l1"), ("pred_noise", "l2"), ("pred_x0", "l1"), ("pred_x0", "l2")])
def test_objectives_and_loss_types(default_net, objective, loss_type):
    _check_case(default_net, _inputs_for(default_net, 3, 5), objective, loss_type, label=f"default (3, 5) {objective} {loss_type}")


@pytest.mark.parametrize("shape", [(3, 7), (9, 15)], ids=["b3n7", "b9n15"])
def test_non_default_cfg_gradients_vs_fp64(small_net, shape):
    _check_case(small_net, _inputs_for(small_net, *shape), "pred_noise", "l1", label=f"{NONDEFAULT.name} {shape}")


def test_bitwise_reproducible_and_independent_of_capacity(default_net):
    inp = _inputs(7, 19)
    exact, big = default_net.trainer("pred_noise", 7, 19), default_net.trainer("pred_noise", 64, 64)
    _, _, a = _engine_pass(exact, default_net, inp, "l1")
    _, _, b = _engine_pass(exact, default_net, inp, "l1")
    _, _, c = _engine_pass(big, default_net, inp, "l1")
    for n in a:
        assert torch.equal(a[n], b[n]), (n, "second run")
        assert torch.equal(a[n], c[n]), (n, "capacity (64, 64)")


def test_selective_gradients(default_net):
    inp = _inputs(3, 5)
    tr = default_net.trainer("pred_noise", 3, 5)
    _, _, full = _engine_pass(tr, default_net, inp, "l1")
    skip = {"_first.weight", "_trunk.layers.3.linear1.weight", "z"}
    _, _, part = _engine_pass(tr, default_net, inp, "l1", want=[n for n in full if n not in skip])
    assert set(part) == set(full) - skip
    for n in part:
        assert torch.equal(part[n], full[n]), n


def test_refusals_leave_a_usable_trainer(default_net):
    bufs = diffusion_buffers()
    with pytest.raises(RuntimeError, match=r"code -2.*pre-norm only"):
        PoseTrainer(dict(default_net.shape, norm_first=False), bufs, 2, 4, device=torch.device(DEV))
    with pytest.raises(RuntimeError, match=r"code -2.*head dim of at most 128"):
        PoseTrainer(dict(default_net.shape, d_model=256, nhead=1), bufs, 2, 4, device=torch.device(DEV))
    tr = default_net.trainer("pred_noise", 2, 65)
    with pytest.raises(RuntimeError, match=r"code -2.*limit of 64 frames"):
        tr.forward(default_net.gpu, **{k: v for k, v in _inputs(2, 65).items()})
    with pytest.raises(RuntimeError, match=r"code -4.*no forward is pending"):
        tr.backward(default_net.gpu, torch.zeros(2, 64, 9, device=DEV))
    # the C entry point itself, with valid pointers
    lib, g = _lib.load(), torch.zeros(2 * 64 * 9, device=DEV)
    assert lib.pd_train_backward(tr._h, C.byref(tr._weights_struct(default_net.gpu)), g.data_ptr(), C.byref(_lib.pd_weight_grads()), None, None) == -4
    assert "no forward is pending" in _lib.last_error()
    inp = _inputs(2, 64)
    _, _, a = _engine_pass(tr, default_net, inp, "l1")                       # a valid call after each refusal
    _, _, b = _engine_pass(default_net.trainer("pred_noise", 2, 64), default_net, inp, "l1")
    assert all(torch.equal(a[n], b[n]) for n in a)
    with pytest.raises(RuntimeError, match=r"code -4.*no forward is pending"):   # a stash is consumed once
        tr.backward(default_net.gpu, torch.zeros(2, 64, 9, device=DEV))


def test_out_of_range_timestep_is_clamped_and_reported(default_net):
    inp = _inputs(3, 5)
    tr = default_net.trainer("pred_noise", 3, 5)
    bad = tr.forward(default_net.gpu, inp["x_start"], inp["z"], torch.tensor([-1, 100, 3]), inp["noise"], "l2")
    with pytest.raises(RuntimeError, match="timestep outside"):
        tr.check_async()
    tr.check_async()
    good = tr.forward(default_net.gpu, inp["x_start"], inp["z"], torch.tensor([0, 99, 3]), inp["noise"], "l2")
    tr.check_async()
    assert all(torch.equal(bad[k], good[k]) for k in bad)


# ------------------------------------------------------------------------------------------------ live weights through the drop-in
def _module_grads_vs_fp64(diff, tr, inp, z_grad=None):
    """.grad of every denoiser parameter against the forced-mask float64 helper at the CURRENT state dict (4 x own)."""
    sd = {k: v.detach().cpu().clone() for k, v in diff.model.state_dict().items()}
    net = TC.DEFAULT_NET
    masks = [tr.debug_relu(l).cpu() > 0 for l in range(net.layers + 1)]
    own64 = TC.loss_and_grads(sd, net, inp, diff.objective, diff.loss_type, want=[])
    r64 = TC.loss_and_grads(sd, net, inp, diff.objective, diff.loss_type, masks=masks, signs=own64["signs"])
    r32 = TC.loss_and_grads(sd, net, inp, diff.objective, diff.loss_type, masks=masks, signs=own64["signs"], dtype=torch.float32)
    misses = []
    got = {n: p.grad for n, p in diff.model.named_parameters()}
    if z_grad is not None:
        got["z"] = z_grad
    for n, g in got.items():
        assert g is not None, n
        e, own = TC.grad_dist(g, r64["grads"][n]), TC.grad_dist(r32["grads"][n], r64["grads"][n])
        if e > RECORDED_MARGIN.get(n, MARGIN) * own:
            misses.append((n, e, own))
    assert not misses, misses
    return own64, r32


def test_dropin_engine_grad_with_live_weights():
    diff = synth.make_diffuser(seed=0)
    synth.randomize_norm_and_bias_(diff.model)
    diff = diff.to(DEV).eval()
    inp = _inputs(3, 5)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    plain = diff.p_losses(dev["x_start"], dev["t"], z=dev["z"], noise=dev["noise"])                     # 8. the default: nothing requires grad
    assert not any(v.requires_grad for v in plain.values())
    diff.model.__dict__.pop("_pd_engine_cache")["e"][1].close()                                        # from here on no engine may appear
    diff.engine_grad = True
    with torch.no_grad():
        assert not diff.p_losses(dev["x_start"], dev["t"], z=dev["z"], noise=dev["noise"])["loss"].requires_grad
    diff.model.__dict__.pop("_pd_engine_cache")["e"][1].close()
    r = diff.p_losses(dev["x_start"], dev["t"], z=dev["z"], noise=dev["noise"])
    assert sorted(r) == ["loss", "noise", "t", "x_0_pred", "x_t"]
    assert r["loss"].requires_grad and not r["x_0_pred"].requires_grad and not r["x_t"].requires_grad
    for k in ("loss", "x_0_pred", "x_t"):                                                               # the same numbers as the forward-only engine, to rounding
        assert TC.grad_dist(r[k], plain[k]) < 2e-5, k
    tr = host.get_trainer(diff.model, diff, 3, 5)
    r["loss"].mean().backward()                                                                         # 2.
    _module_grads_vs_fp64(diff, tr, inp)
    opt = torch.optim.SGD(diff.model.parameters(), lr=0.2)
    opt.step()                                                                                          # 3.
    opt.zero_grad(set_to_none=True)
    z = dev["z"].clone().requires_grad_()
    r2 = diff.p_losses(dev["x_start"], dev["t"], z=z, noise=dev["noise"])                               # 4. the loss of the UPDATED weights
    assert host.get_trainer(diff.model, diff, 3, 5) is tr and "_pd_engine_cache" not in diff.model.__dict__
    r2["loss"].mean().backward()
    own64, r32 = _module_grads_vs_fp64(diff, tr, inp, z_grad=z.grad)                                    # 5. z.grad too
    own = TC.grad_dist(r32["loss"], own64["loss"])
    e_new, e_old = TC.grad_dist(r2["loss"], own64["loss"]), TC.grad_dist(r["loss"], own64["loss"])
    print(f"loss after the step: {e_new:.3e} from float64 at the updated weights (own {own:.3e}); the first loss is {e_old:.3e} away")
    assert e_new <= MARGIN * own and e_old > 100 * e_new
    diff.train()                                                                                        # 7. dropout 0.1 under .train()
    with pytest.raises(RuntimeError, match="dropout"):
        diff.p_losses(dev["x_start"], dev["t"], z=dev["z"], noise=dev["noise"])
    diff.eval()


def test_pose_diffusion_model_training_branch_with_engine_grad():
    import numpy as np
    from posediffusion_amd.compat import AttrDict, PerspectiveCameras
    models = synth._dropin()
    cfg = {"pose_encoding_type": "absT_quaR_logFL",
           "IMAGE_FEATURE_EXTRACTOR": AttrDict({"_target_": "models.MultiScaleImageFeatureExtractor", "freeze": False}),
           "DENOISER": AttrDict({"_target_": "models.Denoiser", "TRANSFORMER": AttrDict(synth.TRANSFORMER_CFG)}),
           "DIFFUSER": AttrDict({"_target_": "models.GaussianDiffusion", "beta_schedule": "custom"})}
    torch.manual_seed(0)
    model = models.PoseDiffusionModel(**cfg).to(DEV).eval()
    B, N = 2, 5
    enc = torch.from_numpy(np.concatenate([synth.make_cameras(N, seed=300 + b) for b in range(B)])).float()
    c = O.pose_encoding_to_camera(enc)
    cams = PerspectiveCameras(focal_length=c["focal_length"].to(DEV), R=c["R"].to(DEV), T=c["T"].to(DEV), device=torch.device(DEV))
    z = synth.make_z(B, N).to(DEV)
    out = model(image=None, gt_cameras=cams, training=True, z=z)
    assert not out["loss"].requires_grad
    model.diffuser.engine_grad = True
    out = model(image=None, gt_cameras=cams, training=True, z=z)
    assert out["loss"].requires_grad and out["loss"].shape == (B, N, 9)
    out["loss"].mean().backward()
    grads = [p.grad for p in model.diffuser.model.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and any(g.abs().max() > 0 for g in grads)
