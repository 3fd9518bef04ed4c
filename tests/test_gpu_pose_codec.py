"""GPU (-m gpu): camera_to_pose_encoding on the engine (pd_camera_to_pose, PoseEngine.camera_to_pose) against the fp64 restatement of
tests/pose_codec_checks.py evaluated on the fp32-rounded inputs (validated on the CPU by tests/test_pose_codec_checks_cpu.py).

T is copied bitwise; the quaternion and logFL groups are within 1e-5, the decode bound of tests/test_gpu_parity.py.  Where the fp64
real part is below 1e-6 (the 180-degree cases) q and -q are the same answer.  Round trip through pose_to_camera returns R and the
(clamped) focal lengths within 1e-5."""
import pytest
import torch

from conftest import rel_err
from denoiser_cfgs import CONFIGS, build_dropin
from pose_codec_checks import camera_cases, camera_to_pose_encoding
from posediffusion_amd.engine import PoseEngine
from posediffusion_amd.host import denoiser_state
from posediffusion_amd.schedule import diffusion_buffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


@pytest.fixture(scope="module")
def eng():
    den = build_dropin(CONFIGS[4], seed=3)              # the smallest configuration: the codec does not depend on the denoiser
    e = PoseEngine(denoiser_state(den), diffusion_buffers(), device=torch.device(DEV), max_B=1, max_N=2, num_layers=1, nhead=3,
                   norm_first=False, pivot=False)
    yield e
    e.close()


def _check(eng, cams, bias=1.8, fmin=0.1, fmax=20.0):
    R32, T32, f32 = cams["R"].float(), cams["T"].float(), cams["focal"].float()
    enc = eng.camera_to_pose(R32.to(DEV), T32.to(DEV), f32.to(DEV), bias, fmin, fmax).cpu()
    ref = camera_to_pose_encoding(R32.double(), T32.double(), f32.double(), bias, fmin, fmax)
    assert enc.shape == ref.shape and torch.isfinite(enc).all()
    assert torch.equal(enc[:, :3], T32)
    q, qr = enc[:, 3:7].double(), ref[:, 3:7]
    flip = (qr[:, :1].abs() < 1e-6) & ((q + qr).abs().amax(dim=-1, keepdim=True) < (q - qr).abs().amax(dim=-1, keepdim=True))
    q = torch.where(flip, -q, q)
    assert (enc[:, 3] >= 0).all()
    assert rel_err(q, qr) < TOL, (q - qr).abs().max()
    assert rel_err(enc[:, 7:], ref[:, 7:]) < TOL
    return enc


def test_camera_to_pose_on_every_case(eng):
    cams = camera_cases()
    n = cams["R"].shape[0]
    enc = _check(eng, cams)
    # round trip: R and focal back within 1e-5 for focal inside [min, max]; outside they come back clamped
    R, T, F = eng.pose_to_camera(enc.to(DEV))
    assert rel_err(R, cams["R"]) < TOL and torch.equal(T.cpu(), cams["T"].float())
    assert rel_err(F, cams["focal"].clamp(0.1, 20.0)) < TOL
    inside = cams["inside"]
    assert inside.sum() == n - 4 and rel_err(F.cpu()[inside], cams["focal"][inside]) < TOL
    assert rel_err(F.cpu()[~inside], torch.tensor([[0.1, 1.0], [2.0, 0.1], [20.0, 3.0], [20.0, 0.1]])) < TOL
    assert float(F.min()) >= 0.1 * (1 - TOL) and float(F.max()) <= 20.0


def test_camera_to_pose_non_default_parameters(eng):
    cams = camera_cases()
    enc = _check(eng, cams, bias=0.7, fmin=0.5, fmax=4.0)
    R, T, F = eng.pose_to_camera(enc.to(DEV), 0.7, 0.5, 4.0)
    assert rel_err(R, cams["R"]) < TOL and rel_err(F, cams["focal"].clamp(0.5, 4.0)) < TOL
    assert float(F.min()) >= 0.5 * (1 - TOL) and float(F.max()) <= 4.0 * (1 + TOL)


@pytest.mark.parametrize("n", [1, 257])
def test_camera_to_pose_sizes(eng, n):
    """One camera, and one block of 256 threads plus one."""
    cams = camera_cases(n_repeat=4)
    cams = {k: v[:n] if n > 1 else v[66:67] for k, v in cams.items()}          # (66: 180 degrees about y, a non-real candidate)
    assert cams["R"].shape[0] == n
    guard = torch.full((n + 1, 9), 7.0, device=DEV)                              # nothing is written past camera n - 1
    enc = _check(eng, cams)
    from posediffusion_amd import _lib
    R32, T32, f32 = cams["R"].float().reshape(-1, 9).to(DEV), cams["T"].float().to(DEV), cams["focal"].float().to(DEV)
    _lib.check(eng.lib.pd_camera_to_pose(R32.data_ptr(), T32.data_ptr(), f32.data_ptr(), n, 1.8, 0.1, 20.0, guard.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "pd_camera_to_pose")
    assert torch.equal(guard[:n].cpu(), enc) and (guard[n] == 7.0).all()


def test_dropin_camera_to_pose_encoding(eng):
    from posediffusion_amd import synth
    from posediffusion_amd.compat import PerspectiveCameras
    synth._dropin()
    from util.camera_transform import camera_to_pose_encoding as dropin_encode, pose_encoding_to_camera
    cams = camera_cases()
    cam = PerspectiveCameras(focal_length=cams["focal"].float().to(DEV), R=cams["R"].float().to(DEV), T=cams["T"].float().to(DEV),
                             device=torch.device(DEV))
    enc = dropin_encode(cam, engine=eng)
    assert torch.equal(enc, eng.camera_to_pose(cam.R, cam.T, cam.focal_length))
    back = pose_encoding_to_camera(enc, engine=eng)
    assert rel_err(back.R, cams["R"]) < TOL
    with pytest.raises(ValueError, match="Unknown pose encoding"):
        dropin_encode(cam, pose_encoding_type="nope", engine=eng)
