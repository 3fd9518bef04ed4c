"""GPU (-m gpu): the drop-in faces of the camera-normalisation kernel -- ``util.normalize_cameras`` under the reference's names on the
project's ``PerspectiveCameras`` (bitwise the batch API, the reference's return shapes) and ``PoseDiffusionModel.forward(normalize_gt=)``
(bitwise the same call on cameras normalised beforehand; ``None`` is today's path)."""
import pytest
import torch

import normalize_checks as NC
from posediffusion_amd import cameras, synth
from posediffusion_amd.compat import AttrDict, PerspectiveCameras

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cams(N, seed, B=1):
    Rs, Ts = zip(*[NC.ring(N, 0.3, seed + b) for b in range(B)])
    R, T = torch.cat(Rs).float().to(DEV), torch.cat(Ts).float().to(DEV)
    g = torch.Generator().manual_seed(seed)
    fl, pp = (torch.rand(B * N, 2, generator=g) * 2 + 1).to(DEV), (torch.rand(B * N, 2, generator=g) * 0.2).to(DEV)
    return PerspectiveCameras(focal_length=fl, principal_point=pp, R=R, T=T, device=torch.device(DEV))


@pytest.fixture(scope="module")
def nc():
    synth._dropin()
    import util.normalize_cameras as m
    return m


def test_reference_named_functions_equal_the_batch_api(nc):
    cam = _cams(20, 1)
    R, T = cam.R[None], cam.T[None]
    for kw in (dict(), dict(compute_optical=False), dict(first_camera=False, normalize_T=True), dict(normalize_T=True)):
        new = nc.normalize_cameras(cam, **kw)                              # co3d_v2.py:332-334 is the first of these
        ref = cameras.normalize_cameras_batch(R, T, **kw)
        assert new is not cam and type(new) is type(cam) and new.R.shape == (20, 3, 3) and new.T.shape == (20, 3)
        assert torch.equal(new.R, ref.R[0]) and torch.equal(new.T, ref.T[0])
        assert torch.equal(new.focal_length, cam.focal_length) and torch.equal(new.principal_point, cam.principal_point)
    assert torch.equal(nc.normalize_cameras(cam, scale=3.0).T, nc.normalize_cameras(cam).T)      # `scale` is dead, as in the reference
    for ro in (False, True):
        new = nc.first_camera_transform(cam, rotation_only=ro)
        ref = cameras.normalize_cameras_batch(R, T, compute_optical=None, first_camera=True, rotation_only=ro)
        assert torch.equal(new.R, ref.R[0]) and torch.equal(new.T, ref.T[0])
        assert torch.equal(new.T, cam.T) == ro
    new = nc.normalize_Trans(cam)
    ref = cameras.normalize_cameras_batch(R, T, compute_optical=None, first_camera=False, normalize_T=True)
    assert torch.equal(new.R, cam.R) and torch.equal(new.T, ref.T[0])
    p, dist, foot, pp2, r = nc.compute_optical_axis_intersection(cam)
    ref = cameras.normalize_cameras_batch(R, T, first_camera=False, diagnostics=True)
    assert p.shape == (1, 3) and dist.shape == (1, 1, 20) and foot.shape == (1, 1, 20, 3) and pp2.shape == (20, 3) and r.shape == (1, 1, 20, 3)
    assert torch.equal(p, ref.p_intersect) and torch.equal(dist[0], ref.dist) and torch.equal(foot[0], ref.foot) and torch.equal(r[0], ref.axis)
    C64, r64 = NC.axes(cam.R.cpu().double(), cam.T.cpu().double())
    assert (pp2.cpu().double() - (C64 + cam.R.cpu().double()[:, :, 2])).abs().max() < 4 * NC.ULP32 * 5
    # the extension: B x N cameras in one object
    many = _cams(20, 40, B=3)
    new, res = nc.normalize_cameras_batch(many, batch_size=3, return_result=True)
    ref = cameras.normalize_cameras_batch(many.R.reshape(3, 20, 3, 3), many.T.reshape(3, 20, 3))
    assert new.R.shape == (60, 3, 3) and torch.equal(new.R, ref.R.reshape(60, 3, 3)) and torch.equal(new.T, ref.T.reshape(60, 3))
    assert res.status.tolist() == [0, 0, 0] and torch.equal(res.scale, ref.scale)
    for b in range(3):
        one = nc.normalize_cameras(PerspectiveCameras(focal_length=many.focal_length[b * 20:(b + 1) * 20], R=many.R[b * 20:(b + 1) * 20],
                                                      T=many.T[b * 20:(b + 1) * 20], device=torch.device(DEV)))
        assert torch.equal(one.R, new.R[b * 20:(b + 1) * 20]) and torch.equal(one.T, new.T[b * 20:(b + 1) * 20])
    ragged = nc.normalize_cameras_batch(many, batch_size=3, n_frames=[20, 7, 13])
    assert not ragged.R[27:40].any() and torch.equal(ragged.R[:20], new.R[:20])


def test_degenerate_inputs_raise(nc):
    R, T = NC.parallel(5)
    cam = PerspectiveCameras(focal_length=torch.ones(5, 2), R=R.float(), T=T.float(), device=torch.device(DEV))
    with pytest.raises(ValueError, match="do not determine a point"):
        nc.normalize_cameras(cam)
    with pytest.raises(ValueError, match="do not determine a point"):
        nc.compute_optical_axis_intersection(cam)
    assert torch.equal(nc.normalize_cameras(cam, compute_optical=False, first_camera=False).R, cam.R)   # no point asked for: fine
    bad = PerspectiveCameras(focal_length=torch.ones(5, 2), R=R.float(), T=T.float() * float("nan"), device=torch.device(DEV))
    with pytest.raises(ValueError, match="non-finite"):
        nc.first_camera_transform(bad)


@pytest.fixture(scope="module")
def model():
    models = synth._dropin()
    cfg = {"pose_encoding_type": "absT_quaR_logFL",
           "IMAGE_FEATURE_EXTRACTOR": AttrDict({"_target_": "models.MultiScaleImageFeatureExtractor", "freeze": False}),
           "DENOISER": AttrDict({"_target_": "models.Denoiser", "TRANSFORMER": AttrDict(synth.TRANSFORMER_CFG)}),
           "DIFFUSER": AttrDict({"_target_": "models.GaussianDiffusion", "beta_schedule": "custom"})}
    torch.manual_seed(0)
    return models.PoseDiffusionModel(**cfg).to(DEV).eval()


@pytest.mark.parametrize("counts", [None, [5, 3]], ids=["uniform", "ragged"])
@pytest.mark.parametrize("kw", [dict(), dict(compute_optical=True, first_camera=True, normalize_T=True)], ids=["defaults", "normT"])
def test_normalize_gt_equals_normalising_beforehand(model, nc, counts, kw):
    B, N = 2, 5
    raw = _cams(N, 70, B=B)
    z = synth.make_z(B, N).to(DEV)
    before = nc.normalize_cameras_batch(raw, batch_size=B, n_frames=counts, **kw)
    extra = {} if counts is None else {"n_frames": counts}
    real = torch.ones(B, N, dtype=torch.bool) if counts is None else torch.arange(N)[None] < torch.tensor(counts)[:, None]
    outs, grads = [], []
    probe = model.diffuser.model._first.weight if hasattr(model.diffuser.model, "_first") else next(model.diffuser.model.parameters())
    for engine_grad in (False, True):
        model.diffuser.engine_grad = engine_grad
        try:
            pair = []
            for cams, ng in ((raw, kw), (before, None)):
                torch.manual_seed(3)
                model.zero_grad(set_to_none=True)
                out = model(image=None, gt_cameras=cams, training=True, z=z, normalize_gt=ng, **extra)
                if engine_grad:
                    out["loss"].sum().backward()
                    grads.append(probe.grad.clone())
                pair.append(out)
        finally:
            model.diffuser.engine_grad = False
        a, b = pair
        assert torch.equal(a["t"], b["t"]) and torch.equal(a["loss"], b["loss"]) and a["loss"].requires_grad == engine_grad
        m = real.to(DEV)
        assert torch.equal(a["x_0_pred"][m], b["x_0_pred"][m])            # (padding rows carry no meaning: their encodings are +0 here,
        flat = m.reshape(-1)                                               #  the encoding of a zero matrix there)
        for f in ("R", "T", "focal_length"):
            assert torch.equal(getattr(a["pred_cameras"], f)[flat], getattr(b["pred_cameras"], f)[flat]), f
        if counts is not None:
            assert not a["loss"][~m].any()
        outs.append(a)
    assert torch.equal(grads[0], grads[1]) and grads[0].abs().max() > 0     # .grad of one denoiser tensor, both ways


def test_normalize_gt_none_is_todays_path_and_bad_keywords_are_refused(model):
    B, N = 2, 5
    raw = _cams(N, 90, B=B)
    z = synth.make_z(B, N).to(DEV)
    torch.manual_seed(5)
    a = model(image=None, gt_cameras=raw, training=True, z=z)
    torch.manual_seed(5)
    b = model(image=None, gt_cameras=raw, training=True, z=z, normalize_gt=None)
    from util.camera_transform import camera_to_pose_encoding
    from posediffusion_amd.host import get_engine
    enc = camera_to_pose_encoding(raw, engine=get_engine(model.diffuser.model, model.diffuser, B, N)).reshape(B, N, 9)
    r = model.diffuser.p_losses(enc, a["t"], z=z, noise=a["noise"])
    for k in ("loss", "x_0_pred", "x_t"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], r[k]), k
    torch.manual_seed(5)
    c = model(image=None, gt_cameras=raw, training=True, z=z, normalize_gt={})
    assert not torch.equal(a["x_t"], c["x_t"])                              # the raw cameras are in another gauge
    with pytest.raises(TypeError, match="unknown normalize_cameras keywords"):
        model(image=None, gt_cameras=raw, training=True, z=z, normalize_gt={"first": True})
    with pytest.raises(ValueError, match="training branch"):
        model(image=None, training=False, z=z, normalize_gt={})
