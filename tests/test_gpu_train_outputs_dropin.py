"""GPU (-m gpu): a camera-space loss end to end through the drop-in -- ``GaussianDiffusion.engine_grad_outputs`` (a differentiable
``x_0_pred``), the differentiable ``util.camera_transform.pose_encoding_to_camera`` and ``PoseDiffusionModel.forward(..., training=True)``.

  1. Case b3n5 under pred_noise on the 2-layer default network (seed 0 + randomize_norm_and_bias_):
       total = loss.mean() + sum(w_R R) + sum(w_T T) + sum(w_f focal_length)        fixed drawn weights on the decoded cameras
     ``total.backward()`` fills ``.grad`` of every denoiser parameter (and z.grad) within 4 x the float32 restatement's own distance of
     the float64 yardstick (tests/train_outputs_checks.py, the engine's ReLU masks forced; per tensor and per train_checks.grad_blocks
     block; 16 x for ``time_embed.linear.0.weight``).  Asserted on the float64 run before anything else, so that a change of weights
     cannot hollow the test out: min |q|^2 of x_0_pred >= 1, a clamped share of the focal entries in [0.25, 0.75], and no focal entry
     closer than 1 % to a clamp edge (measured: 1.94, 0.50, 17 %).
  2. Opt-in off (``engine_grad`` alone): x_0_pred and the decoded cameras carry no grad and ``loss.mean().backward()`` gives the bits of
     pd_train_backward.
  3. Both trainers opted in, through PoseDiffusionModel: pred_cameras' R, T and focal_length carry grad; the backbone's gradients differ
     from the loss-only ones and are bitwise VitTrainer.backward of the dz that PoseTrainer.backward(g_loss, g_x0_pred) returns."""
import pytest
import torch

from p_losses_cases import inputs as case_inputs
import test_gpu_train_grad as G
from test_gpu_vit_train import SMALL_SCALES, _cameras, _model
import train_checks as TC
import train_outputs_checks as TO
from posediffusion_amd import _lib, host, synth
from posediffusion_amd.vit_train import token_rows

pytestmark = pytest.mark.gpu
DEV = G.DEV
MARGIN, RECORDED_MARGIN = G.MARGIN, G.RECORDED_MARGIN
NET2 = TC.Net(2, 4, True)


def _diffuser():
    diff = synth.make_diffuser(seed=0, num_layers=2)
    synth.randomize_norm_and_bias_(diff.model)
    sd = {k: v.detach().clone() for k, v in diff.model.state_dict().items() if v.is_floating_point()}
    return diff.to(DEV).eval(), sd


def _functional(cams, w):
    return sum((w[k].to(DEV) * getattr(cams, k)).sum() for k in ("R", "T", "focal_length"))


def test_camera_space_total_reaches_every_denoiser_parameter():
    from util.camera_transform import pose_encoding_to_camera
    diff, sd = _diffuser()
    assert diff.objective == "pred_noise" and diff.loss_type == "l1"
    inp = case_inputs(1)
    B, N, _ = inp["x_start"].shape
    g_loss = torch.full((B, N, 9), 1.0 / (B * N * 9))
    cam_w = TO.draw_camera_weights(B * N)
    own64 = TO.outputs_and_grads(sd, NET2, inp, "pred_noise", "l1", g_loss=g_loss, cam_w=cam_w, want=[])
    q2 = (own64["x_0_pred"][..., 3:7] ** 2).sum(-1).min().item()
    share, dist = TO.focal_edge_distance(own64["x_0_pred"])
    print(f"float64 x_0_pred: min |q|^2 {q2:.3f}, clamped share of the focal entries {share:.2f}, nearest entry {dist:.2%} from a clamp edge")
    assert q2 >= 1.0 and 0.25 <= share <= 0.75 and dist >= 0.01
    diff.engine_grad = diff.engine_grad_outputs = True
    dev = {k: v.to(DEV) for k, v in inp.items()}
    z = dev["z"].clone().requires_grad_(True)
    r = diff.p_losses(dev["x_start"], dev["t"], z=z, noise=dev["noise"])
    assert sorted(r) == ["loss", "noise", "t", "x_0_pred", "x_t"]
    assert r["loss"].requires_grad and r["x_0_pred"].requires_grad and not r["x_t"].requires_grad
    cams = pose_encoding_to_camera(r["x_0_pred"], engine=host.get_engine(diff.model, diff, B, N))
    assert cams.R.requires_grad and cams.T.requires_grad and cams.focal_length.requires_grad
    tr = host.get_trainer(diff.model, diff, B, N)
    masks = [tr.debug_relu(l).cpu() > 0 for l in range(NET2.layers + 1)]
    (r["loss"].mean() + _functional(cams, cam_w)).backward()
    kw = dict(g_loss=g_loss, cam_w=cam_w, masks=masks, signs=own64["signs"])
    r64 = TO.outputs_and_grads(sd, NET2, inp, "pred_noise", "l1", **kw)
    r32 = TO.outputs_and_grads(sd, NET2, inp, "pred_noise", "l1", dtype=torch.float32, **kw)
    got ={n: p.grad for n, p in diff.model.named_parameters()}
    got["z"] = z.grad
    problems, worst = [], (0.0, "", 0.0, 0.0)
    for n, g in got.items():
        assert g is not None and torch.isfinite(g).all(), n
        g, g64, g32 = g.cpu(), r64["grads"][n], r32["grads"][n]
        e, own = TC.grad_dist(g, g64), TC.grad_dist(g32, g64)
        worst = max(worst, (e / max(own, 1e-30), n, e, own))
        if e > RECORDED_MARGIN.get(n, MARGIN) * own:
            print(f"PARITY MISS {n}: engine {e:.3e} own {own:.3e}")
            problems.append((n, e, own))
        problems += TC.block_misses(n, g, g32, g64, 512, 384, MARGIN, RECORDED_MARGIN)
    print(f"total.backward(): worst engine / own = {worst[0]:.2f} ({worst[1]}: engine {worst[2]:.3e}, own {worst[3]:.3e})")
    assert not problems, problems
    # the camera term is in there: the loss-only gradient of the same weights is far outside the bound
    lo64 = TO.outputs_and_grads(sd, NET2, inp, "pred_noise", "l1", g_loss=g_loss, masks=masks, signs=own64["signs"], want=["_last.3.weight"])
    assert TC.grad_dist(lo64["grads"]["_last.3.weight"], r64["grads"]["_last.3.weight"]) > 1e-2


def test_opt_in_off_keeps_the_loss_only_bits():
    from util.camera_transform import pose_encoding_to_camera
    diff, _ = _diffuser()
    inp = case_inputs(1)
    B, N, _ = inp["x_start"].shape
    dev = {k: v.to(DEV) for k, v in inp.items()}
    diff.engine_grad = True
    assert diff.engine_grad_outputs is False
    r = diff.p_losses(dev["x_start"], dev["t"], z=dev["z"], noise=dev["noise"])
    assert r["loss"].requires_grad and not r["x_0_pred"].requires_grad and not r["x_t"].requires_grad
    cams = pose_encoding_to_camera(r["x_0_pred"], engine=host.get_engine(diff.model, diff, B, N))
    assert not (cams.R.requires_grad or cams.T.requires_grad or cams.focal_length.requires_grad)
    r["loss"].mean().backward()
    tr = host.get_trainer(diff.model, diff, B, N)
    params = {k: v.detach() for k, v in diff.model.named_parameters()}
    out = tr.forward(params, dev["x_start"], dev["z"], dev["t"], dev["noise"], "l1")
    assert all(torch.equal(out[k], r[k].detach()) for k in ("loss", "x_0_pred", "x_t"))
    by_hand = tr.backward(params, torch.ones(B, N, 9, device=DEV) / (B * N * 9), list(params))     # pd_train_backward
    differ = [n for n, p in diff.model.named_parameters() if not torch.equal(p.grad, by_hand[n])]
    assert differ == []


def test_camera_space_term_reaches_the_backbone_through_dz():
    from util.camera_transform import camera_to_pose_encoding
    model = _model()
    B, N = 2, 2
    images = torch.rand(B, N, 3, 32, 32, generator=torch.Generator().manual_seed(11)).to(DEV)
    ext, diff = model.image_feature_extractor, model.diffuser
    ext.engine_grad = diff.engine_grad = True
    cams_gt = _cameras(B, N, 700)
    cam_w = TO.draw_camera_weights(B * N)
    vnames = [n for n, _ in ext._net.named_parameters()]
    torch.manual_seed(1)
    out = model(image=images, gt_cameras=cams_gt, training=True)
    pc = out["pred_cameras"]
    assert not out["x_0_pred"].requires_grad and not (pc.R.requires_grad or pc.T.requires_grad or pc.focal_length.requires_grad)
    out["loss"].mean().backward()
    loss_only = {n: p.grad.clone() for n, p in ext._net.named_parameters()}
    model.zero_grad(set_to_none=True)
    diff.engine_grad_outputs = True
    torch.manual_seed(1)
    out = model(image=images, gt_cameras=cams_gt, training=True)
    pc = out["pred_cameras"]
    assert out["x_0_pred"].requires_grad and pc.R.requires_grad and pc.T.requires_grad and pc.focal_length.requires_grad
    (out["loss"].mean() + _functional(pc, cam_w)).backward()
    grads = {n: p.grad for n, p in ext._net.named_parameters()}
    for n in vnames:
        assert grads[n] is not None and torch.isfinite(grads[n]).all() and not torch.equal(grads[n], loss_only[n]), n
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in diff.model.parameters())
    # the same step by hand: VitTrainer.forward -> PoseTrainer.forward -> decode backward -> PoseTrainer.backward (dz) -> VitTrainer.backward
    vtr = host.get_vit_trainer(ext._net, B * N, B * N * token_rows(32, 32, SMALL_SCALES), len(SMALL_SCALES))
    ptr = host.get_trainer(diff.model, diff, B, N)
    vparams = {k: v.detach() for k, v in ext._net.named_parameters()}
    dparams = {k: v.detach() for k, v in diff.model.named_parameters()}
    z = vtr.forward(vparams, images.reshape(B * N, 3, 32, 32), SMALL_SCALES).reshape(B, N, -1)
    eng = host.get_engine(diff.model, diff, B, N)
    x_start = camera_to_pose_encoding(cams_gt, pose_encoding_type=model.pose_encoding_type, engine=eng).reshape(B, N, 9)
    r = ptr.forward(dparams, x_start, z, out["t"], out["noise"], diff.loss_type)
    assert torch.equal(r["loss"], out["loss"].detach()) and torch.equal(r["x_0_pred"], out["x_0_pred"].detach())
    g_x0 = torch.empty(B * N, 9, device=DEV)
    w = {k: v.to(DEV).contiguous() for k, v in cam_w.items()}
    _lib.check(_lib.load().pd_pose_to_camera_backward(r["x_0_pred"].data_ptr(), w["R"].data_ptr(), w["T"].data_ptr(), w["focal_length"].data_ptr(),
                                                      B * N, 1.8, 0.1, 20.0, g_x0.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "pd_pose_to_camera_backward")
    g_loss = torch.full((B, N, 9), 1.0 / (B * N * 9), device=DEV)
    dz = ptr.backward(dparams, g_loss, ["z"], g_x0_pred=g_x0.reshape(B, N, 9))["z"]
    by_hand = vtr.backward(vparams, dz.reshape(B * N, -1))
    differ = [n for n in vnames if not torch.equal(by_hand[n], grads[n])]
    print(f"{len(vnames)} backbone gradients, {len(differ)} differ from the by-hand step")
    assert differ == []
