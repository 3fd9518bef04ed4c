"""GPU (-m gpu): the backward of pose_encoding_to_camera -- pd_pose_to_camera_backward (include/pd_engine_train.h), called directly and
through the drop-in's ``util.camera_transform.pose_encoding_to_camera`` with an input that requires grad.

Inputs: n = 1, 63, 64, 65 and 200 cameras (both sides of the 64-thread block); quaternions of pose_codec_checks.rotation_cases() scaled
by 0.3, 1 and 3 (quaternion_to_matrix does not normalise: two_s = 2 / |q|^2); logFL so that the focal length lands below the minimum,
inside the range and above the maximum; once with non-default (bias, min, max).  Asserted on float64 alone, before the engine runs:
|q|^2 >= 0.05, and every focal entry at least 1e-3 (relative) from either clamp edge, so fp32 and fp64 take the same clamp branch.

Checks: columns 0-2 are bitwise g_T; clamped focal entries are exactly 0; the quaternion and the logFL columns are each within 4 x the
float32 restatement's own distance of float64 autograd of O.pose_encoding_to_camera (max|g - g64| / max|g64| per column group); a NULL
upstream gives the bits of a zero one.  Every figure is printed before it is asserted."""
import math

import pytest
import torch

from pose_codec_checks import rotation_cases
import train_checks as TC
import train_outputs_checks as TO
from posediffusion_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 4.0
NON_DEFAULT = (0.7, 0.5, 6.0)                     # bias, min, max


def _case(n, focal):
    """enc [n, 9] float32 and the three upstreams (float32, CPU)"""
    bias, lo, hi = focal
    g = torch.Generator().manual_seed(6100 + n)
    q = torch.stack([c[1] for c in rotation_cases()])
    idx = torch.arange(n) % q.shape[0]
    scale = torch.tensor([0.3, 1.0, 3.0], dtype=torch.float64)[(torch.arange(n) // q.shape[0] + torch.arange(n)) % 3]
    quat = q[idx] * scale[:, None]
    # focal targets: below the minimum, inside, above the maximum -- the two entries of a camera take different branches in turn
    rel = torch.tensor([0.3, 0.8, 1.25, 3.0], dtype=torch.float64)
    pick = torch.randint(0, 6, (n, 2), generator=g)
    target = torch.where(pick < 2, lo * rel[pick.clamp(max=1)], torch.where(pick < 4, hi * rel[(pick - 2).clamp(0, 1) + 2],
                                                                            math.sqrt(lo * hi) * (1.0 + 0.2 * (pick - 4).double())))
    if n >= 3:
        target[0], target[1], target[2] = torch.tensor([lo * 0.5, 1.0]), torch.tensor([hi * 2.0, lo * 0.9]), torch.tensor([2.0, hi * 1.1])
    enc = torch.cat([3.0 * torch.randn(n, 3, generator=g, dtype=torch.float64), quat, target.log() - bias], dim=1).float()
    return enc, torch.randn(n, 3, 3, generator=g), torch.randn(n, 3, generator=g), torch.randn(n, 2, generator=g)


def _backward(enc, g_R, g_T, g_f, focal, guard=64):
    """pd_pose_to_camera_backward on the device -> g_enc [n, 9] on the CPU; the output sits between guard floats that must stay untouched"""
    n = enc.shape[0]
    dev = [None if t is None else t.to(DEV).contiguous() for t in (enc, g_R, g_T, g_f)]
    buf = torch.full((n * 9 + 2 * guard,), 7.5, device=DEV)
    out = buf[guard:guard + n * 9]
    _lib.check(_lib.load().pd_pose_to_camera_backward(dev[0].data_ptr(), *(None if t is None else t.data_ptr() for t in dev[1:]), n,
                                                      *focal, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "pd_pose_to_camera_backward")
    torch.cuda.synchronize()
    assert (buf[:guard] == 7.5).all() and (buf[guard + n * 9:] == 7.5).all(), "wrote outside g_enc_out"
    return out.reshape(n, 9).cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n,focal", [(1, TO.FOCAL), (63, TO.FOCAL), (64, TO.FOCAL), (65, TO.FOCAL), (200, TO.FOCAL), (65, NON_DEFAULT)],
                         ids=["n1", "n63", "n64", "n65", "n200", "n65_non_default"])
def test_decode_backward_vs_fp64(n, focal):
    enc, g_R, g_T, g_f = _case(n, focal)
    bias, lo, hi = focal
    # preconditions, on float64 of the fp32 inputs alone
    q2 = (enc[:, 3:7].double() ** 2).sum(-1)
    share, dist = TO.focal_edge_distance(enc, focal)
    print(f"n={n}: min |q|^2 {q2.min().item():.3f}, clamped share {share:.2f}, nearest focal entry {dist:.2e} from a clamp edge")
    assert q2.min().item() >= 0.05 and dist >= 1e-3
    f64 = (enc[:, 7:9].double() + bias).exp()
    clamped = (f64 < lo) | (f64 > hi)
    if n >= 3:
        assert (f64 < lo).any() and (f64 > hi).any() and (~clamped).any()
    g64 = TO.decode_grads(enc, g_R, g_T, g_f, torch.float64, focal)
    g32 = TO.decode_grads(enc, g_R, g_T, g_f, torch.float32, focal)
    g = _backward(enc, g_R, g_T, g_f, focal)
    assert torch.isfinite(g).all()
    assert torch.equal(_bits(g[:, :3]), _bits(g_T)), "columns 0-2 are g_T, copied"
    assert (g[:, 7:9][clamped] == 0).all() and (g64[:, 7:9][clamped] == 0).all()
    problems = []
    for name, sl in (("quaternion", slice(3, 7)), ("logFL", slice(7, 9))):
        e, own = TC.grad_dist(g[:, sl], g64[:, sl]), TC.grad_dist(g32[:, sl], g64[:, sl])
        print(f"n={n} {name}: engine {e:.3e} own {own:.3e} ({e / max(own, 1e-30):.2f} x)")
        if e > MARGIN * own:
            problems.append((name, e, own))
    assert not problems, problems
    # a NULL upstream is a zero upstream, bit for bit
    zR, zT, zf = torch.zeros_like(g_R), torch.zeros_like(g_T), torch.zeros_like(g_f)
    for label, null, zero in (("g_R", (None, g_T, g_f), (zR, g_T, g_f)), ("g_T", (g_R, None, g_f), (g_R, zT, g_f)), ("g_focal", (g_R, g_T, None), (g_R, g_T, zf)),
                              ("g_R and g_focal", (None, g_T, None), (zR, g_T, zf))):
        assert torch.equal(_bits(_backward(enc, *null, focal)), _bits(_backward(enc, *zero, focal))), label
    only_R = _backward(enc, g_R, None, None, focal)
    assert (only_R[:, :3] == 0).all() and (only_R[:, 7:9] == 0).all() and torch.equal(_bits(only_R[:, 3:7]), _bits(g[:, 3:7]))


def test_all_null_upstreams_are_refused():
    enc = torch.zeros(2, 9, device=DEV)
    out = torch.empty(2, 9, device=DEV)
    assert _lib.load().pd_pose_to_camera_backward(enc.data_ptr(), None, None, None, 2, 1.8, 0.1, 20.0, out.data_ptr(), None) == -1
    assert "pd_pose_to_camera_backward" in _lib.last_error() and "all NULL" in _lib.last_error()


def test_drop_in_decode_carries_grad_only_when_asked(engine):
    """util.camera_transform.pose_encoding_to_camera: grad mode on and an input that requires grad -> R, T and focal_length carry grad and
    ``backward`` is pd_pose_to_camera_backward's bits; otherwise exactly the plain decode."""
    from util.camera_transform import pose_encoding_to_camera
    enc, g_R, g_T, g_f = _case(65, TO.FOCAL)
    dev = enc.to(DEV)
    plain = pose_encoding_to_camera(dev, engine=engine)
    assert not (plain.R.requires_grad or plain.T.requires_grad or plain.focal_length.requires_grad)
    leaf = dev.clone().requires_grad_(True)
    with torch.no_grad():
        assert not pose_encoding_to_camera(leaf, engine=engine).R.requires_grad
    cams = pose_encoding_to_camera(leaf, engine=engine)
    assert cams.R.requires_grad and cams.T.requires_grad and cams.focal_length.requires_grad
    assert all(torch.equal(getattr(cams, k), getattr(plain, k)) for k in ("R", "T", "focal_length"))
    ((cams.R * g_R.to(DEV)).sum() + (cams.T * g_T.to(DEV)).sum() + (cams.focal_length * g_f.to(DEV)).sum()).backward()
    assert torch.equal(_bits(leaf.grad.cpu()), _bits(_backward(enc, g_R, g_T, g_f, TO.FOCAL)))
    # an output nobody used reaches the kernel as a NULL pointer
    leaf.grad = None
    d = pose_encoding_to_camera(leaf, return_dict=True, engine=engine)
    (d["focal_length"] * g_f.to(DEV)).sum().backward()
    assert torch.equal(_bits(leaf.grad.cpu()), _bits(_backward(enc, None, None, g_f, TO.FOCAL)))
