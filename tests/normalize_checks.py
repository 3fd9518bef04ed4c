"""Yardstick of the camera-normalisation kernel (include/pd_engine_cameras.h): a dtype-generic restatement of the
reference's util/normalize_cameras.py, the scenes and the case table of the tests, the bound, and the means to execute the reference's
own file in place (minimal pytorch3d stand-ins) for the committed fixtures.

PyTorch3D row convention, X_view = X_world R + T.  The formulas (reference lines in brackets):
  optical-axis intersection [normalize_cameras.py:24-72]   C_i = -T_i R_i^T;  d_i = third column of R_i (the principal point unprojected at
      depth 1 is the view-space point (0, 0, 1) whatever the intrinsics, :56-63);  r_i = d_i / |d_i| (:30);  A = sum_i (I - r_i r_i^T),
      b = sum_i (I - r_i r_i^T) C_i, p = A^-1 b (:32-35, a 3 x 3 lstsq);  dist_i = |p - C_i| (:70);  foot_i = C_i + ((p - C_i) . r_i) r_i (:44-49).
  normalize_cameras, compute_optical=True [:86-102]   scale = dist_0; scale == 0: T_i /= sqrt(||T||_F), R unchanged (:95-98); otherwise
      T_i <- (p R_i + T_i) / scale, R unchanged (:100-102).     compute_optical=False [:104-106]   T_i /= sqrt(||T||_F).
  first_camera_transform [:132-148]   R_i <- R_0^T R_i;  T_i <- T_i - T_0 R_0^T R_i;  rotation_only: T_i unchanged.
  normalize_Trans [:118-128]   s = clamp(||T[1:]||_F / sqrt(N - 1) / 2, 0.01, 100);  T /= s.  (N = 1: the engine's rule, s = 1.)
Run in fp64 this is the oracle; run in fp32 it stands for the reference's arithmetic.  For comparisons with the kernel the oracle
takes the fp32 inputs upcast, so input rounding is not charged to the kernel.

Status codes are the engine's: 0 normalised, 1 the scale == 0 branch, 2 rank-deficient A, 3 non-finite."""
import importlib.util
import itertools
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT) if ROOT not in sys.path else None
from oracle.ref_stubs import REF_ROOT  # noqa: E402  (PD_REFERENCE_ROOT, or where the build container mounts the reference tree)
REF_FILE = os.path.join(REF_ROOT, "pose_diffusion", "util", "normalize_cameras.py")

RANK_TOL = 1e-10          # smallest Cholesky pivot of A over trace(A) (include/pd_engine_cameras.h states the reasons)
FACTOR = 4.0              # the kernel within 4 x the fp32 restatement's own distance from the fp64 one (tests/test_gpu_vit_tokens.py's factor)
FLOOR_ULPS = 4.0          # ... or 4 fp32 ulps of the group's magnitude where the fp32 run happens to land exactly
ULP32 = 2.0 ** -23
GROUPS = ("R", "T", "p", "scale", "dist", "foot")

# ---- the case table ----
SHAPES_N = (2, 3, 20, 63, 64, 65, 255, 256, 257, 1000)        # wave edge, workgroup-stride edge (256 threads), many strides
BATCHES = (1, 3, 7)
MODES = tuple(itertools.product((0, 1, 2), (0, 1, 2), (0, 1)))  # scale_mode x first_camera x normalize_T (include/pd_engine_cameras.h)
DEFAULT_MODE = (1, 1, 0)                                        # normalize_cameras(compute_optical=True, first_camera=True)
GOLDEN_CASES = (("optical_first_n20", 20, dict(compute_optical=True, first_camera=True, normalize_T=False)),
                ("optical_first_normT_n3", 3, dict(compute_optical=True, first_camera=True, normalize_T=True)),
                ("optical_first_n2", 2, dict(compute_optical=True, first_camera=True, normalize_T=False)),
                ("frob_first_n20", 20, dict(compute_optical=False, first_camera=True, normalize_T=False)),
                ("optical_normT_n3", 3, dict(compute_optical=True, first_camera=False, normalize_T=True)),
                ("frob_normT_n20", 20, dict(compute_optical=False, first_camera=False, normalize_T=True)))


def mode_of(compute_optical=True, first_camera=True, normalize_T=False, rotation_only=False):
    return (1 if compute_optical else 2, 0 if not first_camera else (2 if rotation_only else 1), 1 if normalize_T else 0)


# ---- scenes: (R [N, 3, 3], T [N, 3]) float64 tensors; the callers round to fp32 where the kernel is concerned ----
def _look_at(centers, targets, up=(0.0, 1.0, 0.0)):
    """Rotations whose third column (the optical axis in the world) points from each centre to its target; T = -C R."""
    z = targets - centers
    z = z / np.linalg.norm(z, axis=-1, keepdims=True)
    x = np.cross(np.broadcast_to(np.asarray(up), z.shape), z)
    x = x / np.linalg.norm(x, axis=-1, keepdims=True)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=-1)                              # columns = the camera's axes in the world
    T = -np.einsum("nj,njk->nk", centers, R)
    return torch.from_numpy(R), torch.from_numpy(T)


def ring(N, jitter=0.0, seed=0):
    """Co3D-like: cameras at radius 2 .. 4 around a target, each looking at the target displaced by up to `jitter`."""
    g = np.random.default_rng(seed)
    target = np.array([0.5, -0.3, 1.0])
    phi = np.pi * (np.arange(N) + g.uniform(-0.3, 0.3, N)) / N         # half a turn: two cameras never face each other (collinear axes)
    elev = g.uniform(-0.5, 0.5, N)
    rad = g.uniform(2.0, 4.0, N)
    centers = target + rad[:, None] * np.stack([np.cos(phi) * np.cos(elev), np.sin(elev), np.sin(phi) * np.cos(elev)], axis=-1)
    return _look_at(centers, target + jitter * g.uniform(-1.0, 1.0, (N, 3)))


_AXIS_ROTATIONS = [np.array(m, dtype=np.float64) for m in (
    [[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], [[1, 0, 0], [0, 0, 1], [0, -1, 0]],
    [[0, 1, 0], [-1, 0, 0], [0, 0, 1]], [[0, 0, -1], [0, 1, 0], [1, 0, 0]], [[1, 0, 0], [0, 0, -1], [0, 1, 0]])]


def exact_degenerate(N):
    """Camera 0's centre at the origin, every optical axis through the origin, axis-aligned rotations and dyadic distances: every sum of
    the intersection is exact in fp64 (and fp32), so p == 0 and dist_0 == 0 exactly and the scale == 0 branch is taken."""
    R = np.stack([_AXIS_ROTATIONS[i % len(_AXIS_ROTATIONS)] for i in range(N)])
    t = np.array([0.0 if i == 0 else 0.5 * (1 + i % 8) for i in range(N)])
    centers = -t[:, None] * R[:, :, 2]                              # on the camera's own axis, t behind the origin
    T = -np.einsum("nj,njk->nk", centers, R)
    return torch.from_numpy(R), torch.from_numpy(T)


def parallel(N):
    """One rotation for every camera, centres spread: the axes are exactly parallel."""
    R0, _ = _look_at(np.array([[0.3, -0.2, -3.0]]), np.array([[0.5, 0.4, 1.0]]))
    g = np.random.default_rng(5)
    centers = g.uniform(-1.0, 1.0, (N, 3))
    R = R0.repeat(N, 1, 1)
    return R, -torch.einsum("nj,njk->nk", torch.from_numpy(centers), R)


def near_parallel(N, eps=1e-3):
    """Centres within a unit square, all looking at one point 1 / eps away: the axes are up to eps rad apart."""
    g = np.random.default_rng(6)
    centers = np.concatenate([np.array([[-0.5, 0.0, 0.0], [0.5, 0.0, 0.0]]), np.concatenate([g.uniform(-0.5, 0.5, (N, 2)), np.zeros((N, 1))], 1)])[:N]
    return _look_at(centers, np.array([0.0, 0.0, 1.0 / eps]))


# ---- the restatement ----
def axes(R, T):
    """-> (C [N, 3], r [N, 3])"""
    C = -torch.einsum("nk,njk->nj", T, R)
    d = R[:, :, 2]
    return C, d / d.norm(dim=-1, keepdim=True)


def intersection(R, T):
    """-> dict(p [3], dist [N], foot [N, 3], axis [N, 3], C, A, b, rank_ok)"""
    C, r = axes(R, T)
    P = torch.eye(3, dtype=R.dtype) - r[:, :, None] * r[:, None, :]
    A, b = P.sum(0), torch.einsum("nij,nj->i", P, C)
    # rank: the pivots of the Cholesky factorisation of A against trace(A)
    d0 = A[0, 0]
    l10, l20 = A[0, 1] / d0.sqrt(), A[0, 2] / d0.sqrt()
    d1 = A[1, 1] - l10 * l10
    l21 = (A[1, 2] - l20 * l10) / d1.sqrt()
    d2 = A[2, 2] - l20 * l20 - l21 * l21
    tol = RANK_TOL * A.diagonal().sum()
    rank_ok = bool(d0 > tol) and bool(d1 > tol) and bool(d2 > tol)
    p = torch.linalg.solve(A, b) if rank_ok else torch.zeros(3, dtype=R.dtype)
    e = p - C
    return dict(p=p, dist=e.norm(dim=-1), foot=C + (e * r).sum(-1, keepdim=True) * r, axis=r, C=C, A=A, b=b, rank_ok=rank_ok, P=P)


def normalize(R, T, mode=DEFAULT_MODE, dtype=torch.float64):
    """One sequence through the three stages.  -> dict(R, T, p, scale, dist, foot, axis, status); status 2 / 3: R, T as given."""
    scale_mode, first_camera, normalize_T = mode
    R, T = R.to(dtype), T.to(dtype)
    N = R.shape[0]
    zero3 = torch.zeros(3, dtype=dtype)
    out = dict(R=R, T=T, p=zero3, scale=torch.ones((), dtype=dtype), dist=torch.zeros(N, dtype=dtype), foot=torch.zeros(N, 3, dtype=dtype),
               axis=torch.zeros(N, 3, dtype=dtype), status=0)
    if not (bool(torch.isfinite(R).all()) and bool(torch.isfinite(T).all())):
        return dict(out, status=3)
    root_t = T.norm().sqrt()                                             # sqrt of the Frobenius norm (:96-97, :104-105)
    R1, T1 = R, T
    if scale_mode == 1:
        it = intersection(R, T)
        if not (bool(torch.isfinite(it["A"]).all()) and bool(torch.isfinite(it["b"]).all())):
            return dict(out, status=3)                                       # a zero third column has no direction: 0 / 0
        if not it["rank_ok"]:
            return dict(out, status=2)
        if not bool(torch.isfinite(it["p"]).all()):
            return dict(out, status=3)
        out.update(p=it["p"], dist=it["dist"], foot=it["foot"], axis=it["axis"])
        scale = it["dist"][0]
        if scale == 0:
            if not root_t > 0:
                return dict(out, status=3, p=zero3, dist=out["dist"] * 0, foot=out["foot"] * 0, axis=out["axis"] * 0)
            out.update(status=1, scale=root_t)
            T1 = T / root_t
        else:
            out.update(scale=scale)
            T1 = (it["p"] @ R + T) / scale
    elif scale_mode == 2:
        if not root_t > 0:
            return dict(out, status=3)
        out.update(scale=root_t)
        T1 = T / root_t
    if first_camera:
        R2 = R1[0].T @ R1
        T2 = T1 - T1[0] @ R2 if first_camera == 1 else T1
    else:
        R2, T2 = R1, T1
    if normalize_T and N > 1:
        s = (T2[1:].norm() / (N - 1) ** 0.5 / 2).clamp(0.01, 100)
        T2 = T2 / s
    return dict(out, R=R2, T=T2)


# ---- the bound ----
def group_ratio(got, ref64, ref32, groups=GROUPS):
    """{group: (kernel's distance from the fp64 yardstick) / max(FACTOR x the fp32 yardstick's distance, FLOOR_ULPS fp32 ulps), both
    relative to the group's largest magnitude in the sequence}: the bound holds where every ratio is <= 1."""
    out = {}
    for g in groups:
        r64 = torch.as_tensor(ref64[g]).double().reshape(-1)
        mag = float(r64.abs().max().clamp_min(1e-30))
        d_got = float((torch.as_tensor(got[g]).double().reshape(-1) - r64).abs().max()) / mag
        d_32 = float((torch.as_tensor(ref32[g]).double().reshape(-1) - r64).abs().max()) / mag
        out[g] = d_got / max(FACTOR * d_32, FLOOR_ULPS * ULP32)
    return out


# ---- the reference's own file, executed in place ----
def reference_available():
    return os.path.isfile(REF_FILE)


class _Transform:
    """Row-vector 4 x 4 transforms (points are rows: X' = [X 1] M), as much of pytorch3d's Transform3d as normalize_cameras.py uses."""

    def __init__(self, M):
        self._M = M

    def get_matrix(self):
        return self._M

    def compose(self, other):                                            # self first, then other
        return _Transform(self._M @ other._M)

    def inverse(self):
        return _Transform(torch.inverse(self._M))


def Rotate(R):
    M = torch.eye(4, dtype=R.dtype).repeat(R.shape[0], 1, 1)
    M[:, :3, :3] = R
    return _Transform(M)


def Translate(t):
    M = torch.eye(4, dtype=t.dtype).repeat(t.shape[0], 1, 1)
    M[:, 3, :3] = t
    return _Transform(M)


class StandInCameras:
    """What normalize_cameras.py asks of a pytorch3d PerspectiveCameras (PyTorch3D NDC: x_ndc = fx X / Z + px)."""

    def __init__(self, R, T, focal_length=None, principal_point=None):
        n = R.shape[0]
        self.R, self.T = R, T
        self.focal_length = torch.ones(n, 2, dtype=R.dtype) if focal_length is None else focal_length
        self.principal_point = torch.zeros(n, 2, dtype=R.dtype) if principal_point is None else principal_point

    def __len__(self):
        return self.R.shape[0]

    def clone(self):
        return StandInCameras(self.R.clone(), self.T.clone(), self.focal_length.clone(), self.principal_point.clone())

    def get_world_to_view_transform(self):
        return Rotate(self.R).compose(Translate(self.T))

    def get_camera_center(self):
        return self.get_world_to_view_transform().inverse().get_matrix()[:, 3, :3]

    def unproject_points(self, xy_depth, from_ndc=True, world_coordinates=True):
        """[P, 3] points (x_ndc, y_ndc, depth) through each of the n cameras -> [n, P, 3]"""
        assert from_ndc and world_coordinates
        depth = xy_depth[None, :, 2:]
        xy = (xy_depth[None, :, :2] - self.principal_point[:, None, :]) * depth / self.focal_length[:, None, :]
        view = torch.cat([xy, depth.expand(len(self), -1, -1)], dim=-1)
        return (view - self.T[:, None, :]) @ torch.inverse(self.R)


_ref_module = None


def load_reference_module():
    """util/normalize_cameras.py of the reference tree, executed from where it lies on top of the stand-ins above."""
    global _ref_module
    if _ref_module is not None:
        return _ref_module
    names = ("pytorch3d", "pytorch3d.transforms")
    saved = {k: sys.modules.get(k) for k in names}
    sys.modules["pytorch3d"] = types.ModuleType("pytorch3d")
    tr = types.ModuleType("pytorch3d.transforms")
    tr.Rotate, tr.Translate = Rotate, Translate
    sys.modules["pytorch3d.transforms"] = tr
    try:
        spec = importlib.util.spec_from_file_location("_ref_normalize_cameras", REF_FILE)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    _ref_module = m
    return m


def run_reference(R, T, compute_optical=True, first_camera=True, normalize_T=False, focal_length=None, principal_point=None):
    """-> dict(R, T[, p, dist, foot, axis]) as the reference computes them in the dtype of R"""
    m = load_reference_module()
    cams = StandInCameras(R, T, focal_length, principal_point)
    new = m.normalize_cameras(cams, compute_optical=compute_optical, first_camera=first_camera, normalize_T=normalize_T)
    out = dict(R=new.R, T=new.T)
    if compute_optical:
        p, dist, foot, _, r = m.compute_optical_axis_intersection(cams)
        out.update(p=p.reshape(3), dist=dist.reshape(-1), foot=foot.reshape(-1, 3), axis=r.reshape(-1, 3))
    return out


def golden_inputs(k, N):
    R, T = ring(N, jitter=0.3 if k % 2 else 0.0, seed=100 + k)
    g = np.random.default_rng(200 + k)
    fl = torch.from_numpy(g.uniform(1.0, 3.0, (N, 2))).float()
    pp = torch.from_numpy(g.uniform(-0.2, 0.2, (N, 2))).float()
    return R.float(), T.float(), fl, pp


def make_golden(path=None):
    """tests/golden/normalize_cameras.npz: the fp32 inputs of GOLDEN_CASES and what the reference's file returns for them (fp32, and the
    same file run on the same inputs in fp64).  Data the reference wrote; needs the reference tree."""
    out = {"names": np.array([c[0] for c in GOLDEN_CASES]), "modes": np.array([mode_of(**c[2]) for c in GOLDEN_CASES], dtype=np.int32)}
    for k, (name, N, kw) in enumerate(GOLDEN_CASES):
        R, T, fl, pp = golden_inputs(k, N)
        out[f"c{k}_in_R"], out[f"c{k}_in_T"] = R.numpy(), T.numpy()        # (fl, pp: golden_inputs regenerates them; no output depends on them)
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            res = run_reference(R.to(dt), T.to(dt), focal_length=fl.to(dt), principal_point=pp.to(dt), **kw)
            for key, v in res.items():
                out[f"c{k}_{tag}_{key}"] = v.numpy()
    path = path or os.path.join(GOLDEN, "normalize_cameras.npz")
    np.savez_compressed(path, **out)
    return path


def golden_case(g, k):
    """-> (inputs dict, reference fp32 outputs, reference fp64 outputs, mode) of case k of the loaded fixture"""
    pick = lambda pre: {key[len(pre):]: torch.from_numpy(v) for key, v in g.items() if key.startswith(pre)}   # noqa: E731
    return pick(f"c{k}_in_"), pick(f"c{k}_f32_"), pick(f"c{k}_f64_"), tuple(int(v) for v in g["modes"][k])


# ---- intrinsics helpers (util/camera_transform.py:14-61): the cases of tests/golden/intrinsics_adjust.npz ----
INTRINSICS_CASES = (   # name, image (w, h), crop xyxy, new size (w, h)
    ("landscape_down", (640.0, 480.0), (100.0, 50.0, 500.0, 400.0), (224, 224)),
    ("portrait_up", (300.0, 500.0), (20.0, 30.0, 280.0, 470.0), (448, 672)),
    ("square_same", (256.0, 256.0), (64.0, 64.0, 192.0, 192.0), (256, 256)),
    ("crop_touches_border", (640.0, 480.0), (0.0, 0.0, 640.0, 300.0), (320, 150)),
    ("landscape_up", (320.0, 200.0), (10.0, 0.0, 320.0, 200.0), (1280, 800)),
    ("portrait_down", (480.0, 640.0), (1.0, 2.0, 479.0, 600.0), (120, 161)))


def intrinsics_inputs(k):
    g = np.random.default_rng(300 + k)
    return torch.from_numpy(g.uniform(1.0, 3.0, 2)).float(), torch.from_numpy(g.uniform(-0.3, 0.3, 2)).float()


def run_intrinsics(fns, k):
    """The four results of case k through `fns` (a mapping with the helpers' names): crop then rescale, as the datasets chain them."""
    _, wh, xyxy, new = INTRINSICS_CASES[k]
    fl, pp = intrinsics_inputs(k)
    xywh = fns["bbox_xyxy_to_xywh"](np.array(xyxy, dtype=np.float32))
    bbox = torch.from_numpy(xywh)
    fl_c, pp_c = fns["adjust_camera_to_bbox_crop_"](fl, pp, torch.tensor(wh), bbox)
    fl_s, pp_s = fns["adjust_camera_to_image_scale_"](fl_c, pp_c, bbox[2:], torch.tensor(new, dtype=torch.long))
    return dict(xywh=xywh, fl_crop=fl_c.numpy(), pp_crop=pp_c.numpy(), fl_scale=fl_s.numpy(), pp_scale=pp_s.numpy())


def make_intrinsics_golden(path=None):
    """tests/golden/intrinsics_adjust.npz from the reference's util/camera_transform.py (oracle.ref_stubs.load_reference)."""
    from oracle import ref_stubs
    fns = ref_stubs.load_reference().pose_encoding_to_camera.__globals__
    out = {"names": np.array([c[0] for c in INTRINSICS_CASES])}
    for k in range(len(INTRINSICS_CASES)):
        for key, v in run_intrinsics(fns, k).items():
            out[f"c{k}_{key}"] = v
    path = path or os.path.join(GOLDEN, "intrinsics_adjust.npz")
    np.savez_compressed(path, **out)
    return path


if __name__ == "__main__":
    print(make_golden(), make_intrinsics_golden())
