"""GPU (-m gpu): the backbone trainer -- pd_vit_train_forward / pd_vit_train_backward (include/pd_engine_vit_train.h) through
posediffusion_amd.vit_train.VitTrainer, and the drop-in opt-in ``MultiScaleImageFeatureExtractor.engine_grad``.

Yardstick (tests/vit_train_checks.py): float64 autograd of the restated multi-scale extractor on the CPU; ``own`` is float32 autograd of
the same function.  Nets are vit_oracle.make_vit cut to 1 or 2 blocks (one case keeps all 12), images are torch.rand, g_z is random.
  1. PARITY: z and every gradient tensor -- and the q / k / v rows of attn.qkv, the CLS row and the patch rows of pos_embed separately,
     each against its own float64 maximum -- is at most max(4 x own, 8 x 2^-24) from float64; a block whose float64 gradient is
     identically zero is exactly zero.  The k rows of attn.qkv.bias are mathematically zero and are printed only.
  2. DETERMINISM: twice the same bits; a trainer of larger capacity the same bits; ``want=`` subsets the same bits; alternating with a
     denoiser trainer (PoseTrainer, which launches the same pd_tr_* kernel handles and shares their dynamic-LDS bounds) the same bits.
  3. STATE: one stash -- backward without forward, a second backward and an overtaken autograd node are refused.
  4. LIVE WEIGHTS: an in-place SGD step changes the next forward with no rebuild, and that forward meets rule 1 at the updated weights.
  5. DROP-IN: off by default (bitwise today's ``multiscale``), on with both opt-ins; through PoseDiffusionModel the backbone gradients
     are bitwise VitTrainer.backward of the dz PoseTrainer.backward returns, with batch_repeat of the summed dz.
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from oracle import pd_oracle as O
import test_gpu_train_dropout as GD
import test_gpu_train_grad as G
import train_long_checks as L
import vit_train_checks as VC
from posediffusion_amd import host, synth
from posediffusion_amd.schedule import diffusion_buffers
from posediffusion_amd.train import PoseTrainer
from posediffusion_amd.vit_train import VitTrainer, multiscale_with_grad, shape_from_module, token_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RECORDED_MARGIN = {}              # {"tensor" or "tensor[block]": margin <= 16} once its distances and their cause are in profiles/vit_train_parity.txt

CASES = {
    "three_scales_96": VC.Case(3, 96, 96, VC.THREE, 2),        # 37 / 10 / 5 tokens: every scale resamples the grid; 96 / 3 = 32 exercises the floor rule
    "non_square": VC.Case(2, 48, 32, (1,), 1),                 # 3 x 2 patches: 7 tokens
    "trained_grid": VC.Case(2, 224, 224, (1,), 1),             # 197 tokens: the trained grid; crosses the 64 / 128 / 192 key tiles
    "three_scales_224": VC.Case(2, 224, 224, VC.THREE, 2),     # 197 / 50 / 17 tokens
    "token_limit": VC.Case(1, 240, 272, (1,), 1),              # 15 x 17 patches: 256 tokens
    "one_patch": VC.Case(1, 16, 16, (1,), 1),                  # 2 tokens
    "depth_12": VC.Case(2, 96, 96, VC.THREE, 12),              # the smoke case at full depth
}


class _Net:
    """One cut of the oracle's ViT on both sides: the float32 CPU module (the yardstick differentiates copies of it) and its parameters
    on the GPU (the trainer's live tensors)."""

    def __init__(self, depth):
        self.cpu = VC.make_net(depth)
        self.gpu = {k: v.detach().to(DEV).contiguous() for k, v in self.cpu.named_parameters()}
        self.shape = shape_from_module(self.cpu)
        self._trainers, self._refs = {}, {}

    def trainer(self, max_images, max_rows, max_scales=3):
        key = (max_images, max_rows, max_scales)
        if key not in self._trainers:
            self._trainers[key] = VitTrainer(self.shape, max_images, max_rows, max_scales, device=torch.device(DEV))
        return self._trainers[key]

    def trainer_for(self, case):
        return self.trainer(case.n, case.n * token_rows(case.H, case.W, case.scales), len(case.scales))

    def reference(self, case):
        """(images, g_z, (z64, g64), (z32, g32)) of a case: computed once, shared, never modified."""
        if case not in self._refs:
            images, g_z = VC.inputs(case)
            self._refs[case] = (images, g_z, VC.reference(self.cpu, images, g_z, case.scales, torch.float64),
                                VC.reference(self.cpu, images, g_z, case.scales, torch.float32))
        return self._refs[case]

    def close(self):
        for t in self._trainers.values():
            t.close()


@pytest.fixture(scope="module")
def nets():
    made = {}

    def get(depth):
        if depth not in made:
            made[depth] = _Net(depth)
        return made[depth]
    yield get
    for n in made.values():
        n.close()


def _engine_pass(tr, params, images, g_z, scales, want=None):
    z = tr.forward(params, images.to(DEV), scales)
    grads = tr.backward(params, g_z.to(DEV), want)
    return z.cpu(), {k: v.cpu() for k, v in grads.items()}


def _assert_parity(label, z, grads, ref64, ref32):
    (z64, g64), (z32, g32) = ref64, ref32
    e, own = VC.grad_dist(z, z64), VC.grad_dist(z32, z64)
    print(f"[{label}] z: {e:.3e} from float64 (own {own:.3e}, bound {VC.bound(own):.3e})")
    bad = [("z", e, own)] if e > VC.bound(own) else []
    assert sorted(grads) == sorted(g64)
    for name in g64:
        e, own = VC.grad_dist(grads[name], g64[name]), VC.grad_dist(g32[name], g64[name])
        print(f"[{label}] {name}: {e:.3e} (own {own:.3e}, max|g64| {g64[name].abs().max().item():.3e})")
        for blk, eb, ob, zero in VC.block_dists(name, grads[name], g32[name], g64[name]):
            print(f"[{label}]     [{blk}]: {eb:.3e} (own {ob:.3e}){' zero in float64' if zero else ''}{' -- printed only' if VC.is_k_bias(name, blk) else ''}")
        assert torch.isfinite(grads[name]).all(), name
        bad += VC.misses(name, grads[name], g32[name], g64[name], RECORDED_MARGIN)
    assert not bad, [(n, f"{e:.3e}", f"own {o:.3e}") for n, e, o in bad]


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_every_gradient_against_float64(nets, name):
    case = CASES[name]
    net = nets(case.depth)
    images, g_z, ref64, ref32 = net.reference(case)
    z, grads = _engine_pass(net.trainer_for(case), net.gpu, images, g_z, case.scales)
    _assert_parity(case.label, z, grads, ref64, ref32)


def test_257_tokens_are_refused_with_the_limit_and_the_trainer_stays_usable(nets):
    net = nets(1)
    small = CASES["one_patch"]
    tr = net.trainer(1, 300, 1)
    images, g_z, ref64, ref32 = net.reference(small)
    z = tr.forward(net.gpu, images.to(DEV), small.scales)
    with pytest.raises(RuntimeError, match=r"code -2.*257 tokens per image.*limit is 256 tokens"):
        tr.forward(net.gpu, torch.rand(1, 3, 256, 256, device=DEV), (1,))
    grads = tr.backward(net.gpu, g_z.to(DEV))                         # the refused call left the pending stash as it was
    _assert_parity("after a refusal", z.cpu(), {k: v.cpu() for k, v in grads.items()}, ref64, ref32)
    with pytest.raises(RuntimeError, match=r"code -2.*capacity of 1 images"):
        tr.forward(net.gpu, torch.rand(2, 3, 16, 16, device=DEV), (1,))
    with pytest.raises(RuntimeError, match=r"code -2.*limit of 1 scales"):
        tr.forward(net.gpu, torch.rand(1, 3, 64, 64, device=DEV), (1, 1 / 2))
    with pytest.raises(RuntimeError, match=r"code -2.*capacity of 300 token rows"):
        net.trainer(2, 300, 1).forward(net.gpu, torch.rand(2, 3, 224, 224, device=DEV), (1,))      # 2 x 197 rows
    with pytest.raises(RuntimeError, match=r"code -2.*one whole 16 x 16 patch"):
        tr.forward(net.gpu, torch.rand(1, 3, 16, 16, device=DEV), (1 / 2,))
    with pytest.raises(RuntimeError, match=r"code -1.*scale_factors\[0\]"):
        tr.forward(net.gpu, torch.rand(1, 3, 16, 16, device=DEV), (-1.0,))
    z2 = tr.forward(net.gpu, images.to(DEV), small.scales)
    assert torch.equal(z2, z)
    tr.backward(net.gpu, g_z.to(DEV))


def test_same_bits_twice_at_a_larger_capacity_and_for_want_subsets(nets):
    case = CASES["three_scales_96"]
    net = nets(case.depth)
    images, g_z, _, _ = net.reference(case)
    tr = net.trainer_for(case)
    z, grads = _engine_pass(tr, net.gpu, images, g_z, case.scales)
    z_again, grads_again = _engine_pass(tr, net.gpu, images, g_z, case.scales)
    assert torch.equal(z, z_again) and all(torch.equal(grads[k], grads_again[k]) for k in grads)
    big = net.trainer(case.n + 5, 3 * case.n * token_rows(case.H, case.W, case.scales) + 77, 4)
    z_big, grads_big = _engine_pass(big, net.gpu, images, g_z, case.scales)
    assert torch.equal(z, z_big)
    assert [k for k in grads if not torch.equal(grads[k], grads_big[k])] == []
    for want in (["pos_embed"], ["cls_token", "blocks.1.attn.qkv.bias"], ["patch_embed.proj.weight", "norm.bias", "blocks.0.mlp.fc2.weight"],
                 ["blocks.0.norm1.weight", "blocks.1.mlp.fc1.bias", "blocks.1.attn.proj.weight", "patch_embed.proj.bias"]):
        _, sub = _engine_pass(tr, net.gpu, images, g_z, case.scales, want)
        assert sorted(sub) == sorted(want)                              # a tensor left out has no destination at all: it is not written
        assert [k for k in want if not torch.equal(sub[k], grads[k])] == [], want
    with pytest.raises(KeyError, match="unknown gradient names"):
        tr.forward(net.gpu, images.to(DEV), case.scales)
        tr.backward(net.gpu, g_z.to(DEV), ["blocks.7.norm1.weight"])


def test_alternating_with_a_denoiser_trainer_each_keeps_its_own_bits():
    """One device copy of every pd_tr_* kernel serves both trainers (csrc/pd_train_launch.h), so they share kernel handles and the
    dynamic-LDS bound of each: used in turn in one process, each gives the bits it gives alone.  The backbone side has single-chunk
    reductions that write (scale 1 / 2 runs first) and accumulate (scale 1); the denoiser side runs the key-tiled attention at 65 frames
    with dropout at all four sites, i.e. the DROP = true instantiations the backbone trainer never launches."""
    case = VC.Case(3, 32, 48, (1, 1 / 2), 2)                             # 7 and 2 tokens: 21 + 6 rows
    images, g_z = VC.inputs(case)
    vnet = _Net(case.depth)
    dnet = None
    try:
        vtr = vnet.trainer_for(case)                                    # before any PoseTrainer of this test exists
        z_a, g_a = _engine_pass(vtr, vnet.gpu, images, g_z, case.scales)
        dnet = G._Net(L.make_two())
        inp = G._inputs(1, 65)
        ptr = PoseTrainer(dict(dnet.shape, objective="pred_noise"), diffusion_buffers(), 1, 65, device=torch.device(DEV), max_frames=L.MAX_FRAMES)
        dnet._trainers["alternating"] = ptr                             # closed with dnet
        b = GD._bits(ptr, dnet, inp, **L.CAPACITY_DROP)
        z_again, g_again = _engine_pass(vtr, vnet.gpu, images, g_z, case.scales)
        b_again = GD._bits(ptr, dnet, inp, **L.CAPACITY_DROP)
    finally:
        vnet.close()
        if dnet is not None:
            dnet.close()
    assert L.CAPACITY_DROP["dropout_sites"] == GD.D.ALL and L.CAPACITY_DROP["dropout_p"] > 0
    assert torch.isfinite(z_a).all() and all(torch.isfinite(v).all() and v.abs().max() > 0 for v in g_a.values())
    v_differ = [k for k in g_a if not torch.equal(g_a[k], g_again[k])]
    d_differ = [k for k in b if not torch.equal(b[k], b_again[k])]
    print(f"alternating: backbone {len(g_a)} gradients, differing {v_differ}; denoiser {len(b)} tensors, differing {d_differ}")
    assert torch.equal(z_a, z_again) and v_differ == [] and d_differ == []


def test_one_stash_backward_needs_its_own_forward(nets):
    case = CASES["non_square"]
    net = nets(case.depth)
    images, g_z, _, _ = net.reference(case)
    tr = net.trainer(case.n, case.n * token_rows(case.H, case.W, case.scales) + 1, 2)      # a trainer of its own: nothing is pending on it
    with pytest.raises(RuntimeError, match=r"pd_vit_train_backward failed \(code -4\).*no forward is pending"):
        tr.backward(net.gpu, g_z.to(DEV))
    tr.forward(net.gpu, images.to(DEV), case.scales)
    tr.backward(net.gpu, g_z.to(DEV), ["norm.bias"])
    with pytest.raises(RuntimeError, match=r"code -4.*no forward is pending"):
        tr.backward(net.gpu, g_z.to(DEV), ["norm.bias"])
    mod = VC.make_net(case.depth).to(DEV)
    z1 = multiscale_with_grad(tr, mod, images.to(DEV), case.scales)
    z2 = multiscale_with_grad(tr, mod, images.to(DEV), case.scales)
    assert z1.requires_grad and torch.equal(z1, z2)
    with pytest.raises(RuntimeError, match="VitTrainer keeps ONE activation stash"):
        (z1 * g_z.to(DEV)).sum().backward()
    (z2 * g_z.to(DEV)).sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in mod.parameters())
    with pytest.raises(RuntimeError):                                   # the node was consumed (autograd's own message, or the trainer's)
        (z2 * g_z.to(DEV)).sum().backward()


def test_an_in_place_sgd_step_is_seen_by_the_next_forward(nets):
    case = CASES["three_scales_96"]
    net = nets(case.depth)
    images, g_z, (z64_old, _), _ = net.reference(case)
    mod = VC.make_net(case.depth).to(DEV)
    tr = net.trainer_for(case)
    opt = torch.optim.SGD(mod.parameters(), lr=2e-3)
    z = multiscale_with_grad(tr, mod, images.to(DEV), case.scales)
    (z * g_z.to(DEV)).sum().backward()
    ptrs = [p.data_ptr() for p in mod.parameters()]
    opt.step()
    assert ptrs == [p.data_ptr() for p in mod.parameters()]
    cpu = VC.make_net(case.depth)
    cpu.load_state_dict({k: v.detach().cpu() for k, v in mod.state_dict().items()})
    ref64 = VC.reference(cpu, images, g_z, case.scales, torch.float64)
    ref32 = VC.reference(cpu, images, g_z, case.scales, torch.float32)
    opt.zero_grad(set_to_none=True)
    z_new = multiscale_with_grad(tr, mod, images.to(DEV), case.scales)
    (z_new * g_z.to(DEV)).sum().backward()
    moved = VC.grad_dist(z_new, z64_old)
    print(f"z after the step is {moved:.3e} from float64 at the OLD weights")
    assert moved > 100 * VC.bound(VC.grad_dist(ref32[0], ref64[0]))
    _assert_parity("after an SGD step", z_new.detach().cpu(), {k: p.grad.cpu() for k, p in mod.named_parameters()}, ref64, ref32)


# ------------------------------------------------------------------------------------------------ the drop-in
SMALL_SCALES = [1, 1 / 2]        # 32 x 32 images: 5 and 2 tokens (a third scale of 1 / 3 would leave 10 pixels, less than one patch)


def _model():
    from posediffusion_amd.compat import AttrDict
    models = synth._dropin()
    cfg = {"pose_encoding_type": "absT_quaR_logFL",
           "IMAGE_FEATURE_EXTRACTOR": AttrDict({"_target_": "models.MultiScaleImageFeatureExtractor", "freeze": False, "scale_factors": SMALL_SCALES}),
           "DENOISER": AttrDict({"_target_": "models.Denoiser", "TRANSFORMER": AttrDict(synth.TRANSFORMER_CFG)}),
           "DIFFUSER": AttrDict({"_target_": "models.GaussianDiffusion", "beta_schedule": "custom"})}
    torch.manual_seed(0)
    return models.PoseDiffusionModel(**cfg).to(DEV).eval()


def _cameras(n_seq, N, seed):
    from posediffusion_amd.compat import PerspectiveCameras
    enc = torch.from_numpy(np.concatenate([synth.make_cameras(N, seed=seed + b) for b in range(n_seq)])).float()
    c = O.pose_encoding_to_camera(enc)
    return PerspectiveCameras(focal_length=c["focal_length"].to(DEV), R=c["R"].to(DEV), T=c["T"].to(DEV), device=torch.device(DEV))


def test_drop_in_is_off_by_default_and_when_frozen():
    models = synth._dropin()
    images = torch.rand(3, 3, 48, 64, generator=torch.Generator().manual_seed(3)).to(DEV)
    torch.manual_seed(0)
    ext = models.MultiScaleImageFeatureExtractor(scale_factors=SMALL_SCALES).to(DEV)
    z = ext(images)
    assert z.grad_fn is None and not z.requires_grad and torch.equal(z, ext._engine().multiscale(images, SMALL_SCALES))
    ext.engine_grad = True
    with torch.no_grad():
        assert ext(images).grad_fn is None
    zg = ext(images)
    assert zg.grad_fn is not None and "_pd_vit_trainer_cache" in ext._net.__dict__
    e = VC.grad_dist(zg, z)
    print(f"engine_grad z is {e:.3e} from the inference engine's")
    assert e < 2e-5                                                     # two exact-fp32 engines, summed in different orders
    torch.manual_seed(0)
    frozen = models.MultiScaleImageFeatureExtractor(freeze=True, scale_factors=SMALL_SCALES).to(DEV)
    frozen.engine_grad = True
    zf = frozen(images)
    assert zf.grad_fn is None and torch.equal(zf, z) and "_pd_vit_trainer_cache" not in frozen._net.__dict__


def test_pose_diffusion_model_fills_grad_on_denoiser_and_backbone():
    from util.camera_transform import camera_to_pose_encoding
    model = _model()
    B, N = 2, 2
    images = torch.rand(B, N, 3, 32, 32, generator=torch.Generator().manual_seed(11)).to(DEV)
    ext, diff = model.image_feature_extractor, model.diffuser
    ext.engine_grad = diff.engine_grad = True
    vnames = [n for n, _ in ext._net.named_parameters()]
    for repeat, seed in ((-1, 500), (2, 600)):
        R = max(repeat, 1)
        cams = _cameras(B * R, N, seed)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1)
        out = model(image=images, gt_cameras=cams, training=True, batch_repeat=repeat)
        assert out["loss"].requires_grad and out["loss"].shape == (B * R, N, 9)
        out["loss"].mean().backward()
        for fam, mod in (("denoiser", diff.model), ("backbone", ext._net)):
            for n, p in mod.named_parameters():
                assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, (fam, n)
        # the same step by hand: VitTrainer.forward -> PoseTrainer.forward / backward (dz) -> VitTrainer.backward
        vtr = host.get_vit_trainer(ext._net, B * N, B * N * token_rows(32, 32, SMALL_SCALES), len(SMALL_SCALES))
        ptr = host.get_trainer(diff.model, diff, B * R, N)
        vparams = {k: v.detach() for k, v in ext._net.named_parameters()}
        dparams = {k: v.detach() for k, v in diff.model.named_parameters()}
        z = vtr.forward(vparams, images.reshape(B * N, 3, 32, 32), SMALL_SCALES).reshape(B, N, -1)
        eng = host.get_engine(diff.model, diff, B * R, N)
        x_start = camera_to_pose_encoding(cams, pose_encoding_type=model.pose_encoding_type, engine=eng).reshape(B * R, N, 9)
        zr = z.repeat(R, 1, 1) if repeat > 0 else z
        r = ptr.forward(dparams, x_start, zr, out["t"], out["noise"], diff.loss_type)
        assert torch.equal(r["loss"], out["loss"].detach())
        g_loss = torch.full((B * R, N, 9), 1.0 / (B * R * N * 9), device=DEV)
        dz = ptr.backward(dparams, g_loss, ["z"])["z"]
        g_z = dz.reshape(R, B, N, -1).sum(0) if repeat > 0 else dz              # batch_repeat: z.repeat's backward sums the copies
        by_hand = vtr.backward(vparams, g_z.reshape(B * N, -1))
        differ = [n for n in vnames if not torch.equal(by_hand[n], dict(ext._net.named_parameters())[n].grad)]
        print(f"batch_repeat={repeat}: {len(vnames)} backbone gradients, {len(differ)} differ from the by-hand step")
        assert differ == []
