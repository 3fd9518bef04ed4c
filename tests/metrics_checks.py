"""The evaluation, alignment, preprocessing and decode kernels at their edges (a plain helper module, imported by the tests).

csrc/pd_metrics.hip and pd_camera_kernel / pd_finish_kernel of csrc/pd_engine.hip produce the numbers people read: relative pose errors,
AUC / accuracies, ARE, aligned cameras, the network's input images, decoded cameras.  The earlier tests held them to whole-array bounds of
2e-2 .. 5e-2 degrees on benign inputs.  These helpers give every compared quantity a bound that does not come from the code under test:

    angles from fp32 inputs:   err <= max(K x e32, floor)
        e32    the CPU fp32 oracle's own distance from the fp64 oracle on the same fp32 inputs (one thread), the largest value per BAND
               of the true angle over every case the GPU tests run (`rel_cases`, `are_cases`; `python tests/metrics_checks.py` prints
               the tables below, tests/test_metrics_checks_cpu.py recomputes a subset and asserts it does not exceed them);
        floor  two fp32 ulps of the reference value: an fp32 output cannot be held closer than its own spacing (3e-5 degrees at 180);
        K = 4  as in tests/vit_checks.py: the kernel and the fp32 oracle are two fp32 evaluations of one function that differ in summation
               order and FMA contraction.
    A band is asserted in DEGREES only where K x e32 stays below what the earlier tests assert (2e-2 degrees).  Where acos amplifies 2^-24
    beyond that -- the translation angle of near-coincident directions (acos sqrt(1 - loss) near 1), of near-orthogonal ones (1 - loss is
    rounded at 1 and sqrt amplifies it near 0) and the ARE near 0 (acos of a clipped trace near 1; the folded 180 end lands there too;
    tests/test_metrics_checks_cpu.py asserts 4 x e32 > 2e-2 degrees for all three) -- the asserted quantity is the COSINE form the kernel computes before the acos,
    recomputed in fp64 from the kernel's output: cos^2 of the translation angle, cos of the ARE, under the same rule with that quantity's
    own e32; the angle itself only has to be finite and inside [0, 90] there.

    exact quantities (AUC within 1e-6, accuracies within 1e-4, the bounds of the earlier test): `auc_edge_sensitivity` shows from the fixture
    alone that one misplaced pair moves them by >= 100 x that.  NaN positions compare by mask, the 1e6 default with the floor alone.

Every check returns per-band results (worst index, its (sequence, i, j), error, bound), so that a failure names the edge."""
import contextlib
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

if __name__ == "__main__":          # run as a script: the repository root is not on sys.path yet (under pytest, conftest.py puts it there)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pd_oracle as O  # noqa: E402

K_E32 = 4.0
DEG_FIXTURE, DEG_RANDOM = 2e-2, 5e-2          # what tests/test_gpu_parity.py asserts on fixture / random inputs (degrees)
AUC_TOL, ACC_TOL = 1e-6, 1e-4                 # test_metrics_vs_reference_fixture
ALIGN_R_TOL, ALIGN_T_TOL = 5e-6, 5e-5         # test_camera_alignment_vs_oracle_and_exact_recovery
ALIGN_MIN_COND = 1e-2                         # smallest / largest singular value of the fp64 covariance a compared case must have
PREP_FLOOR = 2e-6                             # test_image_preprocessing_vs_reference_fixture
DECODE_R_FLOOR, DECODE_F_FLOOR = 1e-6, 2e-6   # test_pose_decode_parameters_vs_reference_fixture
ULP1 = float(np.spacing(np.float32(1.0)))
DEFAULT_MIN = 1e5                             # a translation error above this is the 1e6 rad default (5.7e7 degrees)

# (name, lo, hi, quantity) over the fp64 reference angle in degrees, lo <= angle < hi
ROT_BANDS = (("r 0-0.81 (upper extrapolation)", 0.0, 0.81, "deg"), ("r 0.81-5", 0.81, 5.0, "deg"), ("r 5-175", 5.0, 175.0, "deg"),
             ("r 175-179.19", 175.0, 179.19, "deg"), ("r 179.19-180 (lower extrapolation)", 179.19, 181.0, "deg"))
TRA_BANDS = (("t 0-0.5 (near-coincident)", 0.0, 0.5, "cos2"), ("t 0.5-5", 0.5, 5.0, "deg"), ("t 5-89", 5.0, 89.0, "deg"),
             ("t 89-90 (near-orthogonal)", 89.0, 90.001, "cos2"))
ARE_BANDS = (("are 0-2 (both ends of the fold)", 0.0, 2.0, "cos"), ("are 2-88", 2.0, 88.0, "deg"), ("are 88-90 (the fold)", 88.0, 90.001, "deg"))

# Largest e32 per band in the band's quantity (degrees, or the cosine form), CPU fp32 oracle against the fp64 oracle on one thread over all of
# `rel_cases` / `are_cases` / `decode_families` / PREP_CASES; produced by `python tests/metrics_checks.py` and rounded up.
# Measured: r 7.02e-4 / 6.25e-4 / 9.97e-5 / 4.89e-4 / 6.81e-4 degrees; t 3.16e-7 (cos^2) / 7.48e-4 / 5.14e-4 degrees / 3.90e-8 (cos^2);
# ARE 9.97e-8 (cos) / 1.28e-4 / 1.21e-5 degrees.  In degrees the three cosine-form bands measure 2.8e-2 (t near 0), 9.6e-3 (t near 90: the
# reference's 1 - (1 - d^2) is rounded at 1) and 1.2e-2 (ARE near 0): 4 x each of them is beyond the 2e-2 of the earlier tests, hence the cosine form.
E32_ROT = {"r 0-0.81 (upper extrapolation)": 7.5e-4, "r 0.81-5": 7e-4, "r 5-175": 1.1e-4, "r 175-179.19": 5.5e-4,
           "r 179.19-180 (lower extrapolation)": 7.5e-4}
E32_TRA = {"t 0-0.5 (near-coincident)": 3.5e-7, "t 0.5-5": 8e-4, "t 5-89": 5.5e-4, "t 89-90 (near-orthogonal)": 4.5e-8}
E32_ARE = {"are 0-2 (both ends of the fold)": 1.1e-7, "are 2-88": 1.4e-4, "are 88-90 (the fold)": 1.4e-5}
# decode: largest absolute error of a rotation entry per family (n = 1, 257, 100 000), largest relative error of a focal length
E32_DECODE_R = {"norm 1": 4e-7, "norm 1e-3": 4.8e-7, "norm 1e3": 4.2e-7, "negative real part": 4.1e-7, "near identity": 4e-9, "half turn": 4.2e-7}
E32_DECODE_F = 2.5e-7
# preprocessing: torch's fp32 bilinear resize against its fp64 one, largest absolute difference per ((H, W, S), input).  The source index is
# formed in fp32 on both sides; its rounding times the pixel gradient is the whole error, so large frames of random / checkerboard pixels
# cannot be held to 2e-6 by the reference itself, while the ramp (gradient <= 1 / 255) can.
E32_PREP = {
    ((2, 2, 1), "random"): 1.7e-8, ((2, 2, 1), "checkerboard"): 1.7e-8, ((2, 2, 1), "ramp"): 1.1e-8,
    ((2, 2, 7), "random"): 8.3e-8, ((2, 2, 7), "checkerboard"): 8.3e-8, ((2, 2, 7), "ramp"): 8.8e-8,
    ((3, 5, 4), "random"): 6.2e-8, ((3, 5, 4), "checkerboard"): 2e-8, ((3, 5, 4), "ramp"): 7.2e-8,
    ((5, 3, 4), "random"): 6.1e-8, ((5, 3, 4), "checkerboard"): 2e-8, ((5, 3, 4), "ramp"): 7.2e-8,
    ((224, 224, 224), "random"): 3.3e-8, ((224, 224, 224), "checkerboard"): 1.5e-8, ((224, 224, 224), "ramp"): 3.3e-8,
    ((225, 224, 224), "random"): 3.3e-8, ((225, 224, 224), "checkerboard"): 1.5e-8, ((225, 224, 224), "ramp"): 3.3e-8,
    ((224, 225, 224), "random"): 3.3e-8, ((224, 225, 224), "checkerboard"): 1.5e-8, ((224, 225, 224), "ramp"): 3.3e-8,
    ((301, 533, 224), "random"): 1.3e-7, ((301, 533, 224), "checkerboard"): 1.7e-8, ((301, 533, 224), "ramp"): 1.2e-7,
    ((300, 534, 224), "random"): 2.4e-5, ((300, 534, 224), "checkerboard"): 3.8e-5, ((300, 534, 224), "ramp"): 2e-7,
    ((1080, 1920, 224), "random"): 1.25e-4, ((1080, 1920, 224), "checkerboard"): 1.3e-4, ((1080, 1920, 224), "ramp"): 9.3e-7,
    ((3000, 4000, 224), "random"): 3e-4, ((3000, 4000, 224), "checkerboard"): 4.5e-4, ((3000, 4000, 224), "ramp"): 1.7e-6,
    ((64, 48, 336), "random"): 7.4e-6, ((64, 48, 336), "checkerboard"): 8.4e-6, ((64, 48, 336), "ramp"): 1.5e-7,
    ((300, 533, 1), "random"): 3.4e-8, ((300, 533, 1), "checkerboard"): 1e-9, ((300, 533, 1), "ramp"): 4.8e-8,
}


@contextlib.contextmanager
def one_thread():
    """the fp32 oracle, whose rounding IS the yardstick, runs on one CPU thread"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


# ---- angle checks ---------------------------------------------------------------------------------------------------------------------
def _quantity(deg, mode):
    deg = np.asarray(deg, dtype=np.float64)
    if mode == "deg":
        return deg
    c = np.cos(np.deg2rad(deg))
    return c * c if mode == "cos2" else c


def _floor(ref, mode):
    """two fp32 ulps: of the reference angle in degrees; of 1 for the cosine forms, the magnitude at which 1 - d^2, 1 - loss and the trace
    are rounded"""
    if mode == "deg":
        return 2.0 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.full(ref.shape, 2.0 * ULP1)


def pair_of(index, N):
    """flat output index -> (sequence, i, j) in torch.combinations order"""
    P = N * (N - 1) // 2
    i, j = torch.combinations(torch.arange(N), 2)[index % P].tolist()
    return index // P, i, j


def angle_errs(got, ref64, bands, e32, N=None):
    """got (degrees, any float type), ref64 (fp64 degrees) -> one dict per band that has entries: band, mode, n, index of the worst entry
    (largest err / bound), its (sequence, i, j) when N is given, err, bound, got, ref, ok.  NaN entries of `ref64` and the 1e6 default are
    not banded (see `mask_errs`); a non-finite `got` where the reference is finite is an infinite error."""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref64, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    out = []
    usable = np.isfinite(ref) & (ref < DEFAULT_MIN)
    assert all(any(lo <= v < hi for _, lo, hi, _ in bands) for v in ref[usable]), "a reference angle outside every band"
    for name, lo, hi, mode in bands:
        idx = np.nonzero(usable & (ref >= lo) & (ref < hi))[0]
        if not len(idx):
            continue
        g, r = got[idx], ref[idx]
        err = np.abs(_quantity(g, mode) - _quantity(r, mode))
        bad = ~np.isfinite(g) if mode == "deg" else ~(np.isfinite(g) & (g >= 0.0) & (g <= 90.0))
        err = np.where(bad | np.isnan(err), np.inf, err)
        bound = np.maximum(K_E32 * e32[name], _floor(r, mode))
        w = int(np.argmax(err / bound))
        out.append({"band": name, "mode": mode, "n": len(idx), "index": int(idx[w]), "pair": None if N is None else pair_of(int(idx[w]), N),
                    "err": float(err[w]), "bound": float(bound[w]), "got": float(g[w]), "ref": float(r[w]), "ok": bool((err <= bound).all()),
                    "e32_worst": float(err.max())})
    return out


def mask_errs(got, ref64):
    """NaN positions by mask, the 1e6 rad default (5.7e7 degrees) within two fp32 ulps of the reference's value -> list of complaints"""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref64, dtype=np.float64).reshape(-1)
    bad = []
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        bad.append(f"NaN mask differs at {np.nonzero(np.isnan(got) != np.isnan(ref))[0].tolist()[:8]}")
    d = np.nonzero(np.nan_to_num(ref) >= DEFAULT_MIN)[0]
    for k in d:
        if not abs(got[k] - ref[k]) <= 2.0 * float(np.spacing(np.float32(ref[k]))):
            bad.append(f"default at {k}: got {got[k]!r}, reference {ref[k]!r}")
    return bad


def describe(results):
    return "; ".join(f"[{r['band']} | {r['mode']} | n {r['n']} | worst {r['err']:.2e} (bound {r['bound']:.2e}) at {r['index']}"
                     + (f" = (seq {r['pair'][0]}, pair {r['pair'][1]}-{r['pair'][2]})" if r["pair"] else "")
                     + f" got {r['got']:.6f} ref {r['ref']:.6f}]" for r in results)


def failures(results):
    return [r for r in results if not r["ok"]]


# ---- relative pose cases ------------------------------------------------------------------------------------------------------------------
REL_SHAPES = ((1, 2), (1, 3), (3, 5), (256, 20), (2, 50), (1, 128))


def random_cameras(B, N, seed):
    """independent random ground truth and prediction: rotations over all of SO(3), translations N(0, 1); fp32"""
    g = torch.Generator().manual_seed(seed)
    Rg, Rp = (O.quaternion_to_matrix(torch.randn(B * N, 4, generator=g, dtype=torch.float64)).float() for _ in range(2))
    Tg, Tp = torch.randn(B * N, 3, generator=g), torch.randn(B * N, 3, generator=g)
    return Rp, Tp, Rg, Tg


def fixture_rel_case(g, name):
    """one relative-pose case of golden["metrics_edges"] -> dict(Rp, Tp, Rg, Tg, B, r, t) (numpy).  `same` and `turn<k>` share their ground
    truth and translations, which the file stores once."""
    name = str(name)
    if name == "trans":
        return {k: g[f"trans_{k}"] for k in ("Rp", "Tp", "Rg", "Tg", "r", "t")} | {"B": int(g["trans_B"])}
    base = {"Tp": g["base_Tg"], "Rg": g["base_Rg"], "Tg": g["base_Tg"], "B": int(g["base_B"])}
    if name == "same":
        return base | {"Rp": g["base_Rg"], "r": g["same_r"], "t": g["same_t"]}
    k = int(name[len("turn"):])
    return base | {"Rp": g["turn_Rp"][k], "r": g["turn_r"][k], "t": g["turn_t"][k]}


def rel_cases(g):
    """every relative-pose case of the GPU tests: (tag, R_pred, T_pred, R_gt, T_gt, B, N) fp32 CPU tensors; g = golden["metrics_edges"]"""
    for name in g["rel_cases"]:
        c = fixture_rel_case(g, name)
        t = [torch.from_numpy(np.ascontiguousarray(c[k])) for k in ("Rp", "Tp", "Rg", "Tg")]
        yield (f"fixture {name}", *t, c["B"], t[0].shape[0] // c["B"])
    for k, (B, N) in enumerate(REL_SHAPES):
        yield (f"random B {B} N {N}", *random_cameras(B, N, 100 + k), B, N)
    Rp, Tp, Rg, Tg = random_cameras(3, 5, 200)
    for s in (1e-6, 1e6):                     # the `+ eps` of the norms (1e-15) must stay invisible at either scale
        yield (f"random B 3 N 5, translations x {s:g}", Rp, Tp * s, Rg, Tg * s, 3, 5)


def rel_oracle(Rp, Tp, Rg, Tg, B, dtype):
    with one_thread():
        r, t = O.camera_to_rel_deg(Rp.to(dtype), Tp.to(dtype), Rg.to(dtype), Tg.to(dtype), B)
    return r.numpy().astype(np.float64), t.numpy().astype(np.float64)


def are_cases(g):
    """(tag, R_a, R_b) fp32: the fixture's angles, then random pairs over all of SO(3) (82 % of them above 90 degrees) at the block tails"""
    yield "fixture", torch.from_numpy(g["are_Ra"]), torch.from_numpy(g["are_Rb"])
    for n in (1, 127, 128, 129, 10000):
        gen = torch.Generator().manual_seed(300 + n)
        Ra, Rb = (O.quaternion_to_matrix(torch.randn(n, 4, generator=gen, dtype=torch.float64)).float() for _ in range(2))
        yield f"random n {n}", Ra, Rb


def are_oracle(Ra, Rb, dtype):
    return O.compute_ARE(Ra.numpy().astype(dtype), Rb.numpy().astype(dtype)).astype(np.float64)


def unfolded_are(Ra, Rb):
    """fp64 angle of R_a^T R_b before the fold (to count how many pairs a case has above 90 degrees)"""
    tr = np.einsum("bij,bij->b", Ra.numpy().astype(np.float64), Rb.numpy().astype(np.float64))
    return np.degrees(np.arccos(np.clip((tr - 1) / 2, -1, 1)))


def _band_max(table, results):
    for r in results:
        table[r["band"]] = max(table.get(r["band"], 0.0), r["e32_worst"])


def measure_angle_e32(g, only=None):
    """{band: largest e32} for ROT_BANDS, TRA_BANDS, ARE_BANDS over the cases whose tag contains one of `only` (None: all)"""
    zero = {b[0]: 0.0 for b in ROT_BANDS + TRA_BANDS + ARE_BANDS}
    rot, tra, are = {}, {}, {}
    for tag, Rp, Tp, Rg, Tg, B, N in rel_cases(g):
        if only is not None and not any(o in tag for o in only):
            continue
        r32, t32 = rel_oracle(Rp, Tp, Rg, Tg, B, torch.float32)
        r64, t64 = rel_oracle(Rp, Tp, Rg, Tg, B, torch.float64)
        _band_max(rot, angle_errs(r32, r64, ROT_BANDS, zero))
        _band_max(tra, angle_errs(t32, t64, TRA_BANDS, zero))
    for tag, Ra, Rb in are_cases(g):
        if only is not None and not any(o in tag for o in only):
            continue
        _band_max(are, angle_errs(are_oracle(Ra, Rb, np.float32), are_oracle(Ra, Rb, np.float64), ARE_BANDS, zero))
    return rot, tra, are


# ---- summary --------------------------------------------------------------------------------------------------------------------------
def summary_expected(r, t, max_threshold):
    """[Auc, Racc_5, Racc_15, Racc_30, Tacc_5, Tacc_15, Tacc_30] in fp64 from O.calculate_auc_np (pinned to the reference by
    tests/test_oracle_golden.py) and np.mean(err < k) * 100 (test.py:113-119)"""
    r, t = np.asarray(r, dtype=np.float64), np.asarray(t, dtype=np.float64)
    return [O.calculate_auc_np(r, t, max_threshold)] + [float(np.mean(r < k) * 100) for k in (5, 15, 30)] \
        + [float(np.mean(t < k) * 100) for k in (5, 15, 30)]


def summary_errs(got7, exp7):
    """-> list of complaints (AUC within AUC_TOL, accuracies within ACC_TOL)"""
    names = ("Auc", "Racc_5", "Racc_15", "Racc_30", "Tacc_5", "Tacc_15", "Tacc_30")
    return [f"{n}: got {float(a)!r}, expected {float(b)!r}" for n, a, b, tol in zip(names, got7, exp7, (AUC_TOL,) + (ACC_TOL,) * 6)
            if not abs(float(a) - float(b)) <= tol]


def auc_edge_sensitivity(r, t, max_threshold):
    """The smallest change of the expected AUC when ONE pair whose larger error lies in [0, max_threshold] moves to a neighbouring bin or
    out of the histogram, or when a pair the reference drops is binned after all (measured: every such move is tried); and the change of an
    accuracy when one pair crosses its threshold, which is 100 / n by definition of np.mean(err < k) * 100, not a measurement:
    (d_auc, d_acc).  Both must be >= 100 x their tolerance for an edge array to show a single misplaced pair."""
    r, t = np.asarray(r, dtype=np.float64), np.asarray(t, dtype=np.float64)
    base = O.calculate_auc_np(r, t, max_threshold)
    m = np.max(np.stack([r, t], 1), axis=1)
    d_auc = np.inf
    for k in np.nonzero((m >= 0) & (m <= max_threshold))[0]:
        b = min(int(np.floor(m[k])), max_threshold - 1)
        for nb in (b - 1, b + 1):                                    # -1 and max_threshold: out of the histogram (dropped)
            r2, t2 = r.copy(), t.copy()
            r2[k] = t2[k] = nb + 0.5 if 0 <= nb < max_threshold else -1.0
            d_auc = min(d_auc, abs(O.calculate_auc_np(r2, t2, max_threshold) - base))
    for k in np.nonzero(~((m >= 0) & (m <= max_threshold)))[0]:       # a dropped pair (NaN, inf, negative, too large) wrongly binned at 0 or last
        for v in (0.5, max_threshold - 0.5):
            r2, t2 = r.copy(), t.copy()
            r2[k] = t2[k] = v
            d_auc = min(d_auc, abs(O.calculate_auc_np(r2, t2, max_threshold) - base))
    return float(d_auc), 100.0 / len(r)


# ---- alignment ------------------------------------------------------------------------------------------------------------------------
def align_oracle(Rs, Ts, Rt, Tt, estimate_scale, eps):
    """fp64 oracle on the fp32 inputs, eps as the fp32 number the C-ABI receives -> (R, T, s, R_A, T_A, singular values of the covariance)"""
    Rs, Ts, Rt, Tt = (x.double() for x in (Rs, Ts, Rt, Tt))
    R, T, (RA, TA, s) = O.corresponding_cameras_alignment(Rs, Ts, Rt, Tt, estimate_scale=bool(estimate_scale), eps=float(np.float32(eps)))
    sv = torch.linalg.svdvals((Rs @ Rt.transpose(1, 2)).mean(0))
    return R, T, float(s), RA, TA, sv


def similar_cameras(n, seed, scale=0.6, noise=0.0):
    """source cameras and their image under a similarity (s, R_A, T_A), optionally perturbed; fp32"""
    g = torch.Generator().manual_seed(seed)
    R = O.quaternion_to_matrix(torch.randn(n, 4, generator=g, dtype=torch.float64))
    T = torch.randn(n, 3, generator=g, dtype=torch.float64) + torch.tensor([0.0, 0.0, 6.0], dtype=torch.float64)
    RA = O.quaternion_to_matrix(torch.randn(1, 4, generator=g, dtype=torch.float64))[0]
    TA = torch.randn(3, generator=g, dtype=torch.float64)
    Rt = RA.T[None] @ R
    Tt = scale * T - (TA[None, None] @ Rt)[:, 0]
    if noise:
        e1 = torch.tensor([1.0, 0, 0, 0], dtype=torch.float64)
        Rt = O.quaternion_to_matrix(torch.randn(n, 4, generator=g, dtype=torch.float64) * noise + e1) @ Rt
        Tt = Tt + noise * scale * torch.randn(n, 3, generator=g, dtype=torch.float64)
    return R.float(), T.float(), Rt.float(), Tt.float()


def same_A_cameras(n, seed):
    """A_i = R_src_i T_src_i is the same vector for every camera (up to the fp32 rounding of T_src): den ~ 1e-14, far below any eps"""
    R, _, Rt, Tt = similar_cameras(n, seed, noise=0.05)
    a = torch.tensor([0.5, -1.25, 2.0], dtype=torch.float64)
    T = (R.double().transpose(1, 2) @ a[None, :, None])[:, :, 0]
    return R, T.float(), Rt, Tt


def negative_det_cameras(n, seed):
    """R_tgt_k = D_k R_src_k with D_k the half turns about x, y, z in turn, n a multiple of 3: cov = mean R_src R_tgt^T = -I / 3, far from
    singular, determinant negative; V U^T = -I is the orthogonal polar factor, unique although the singular values coincide"""
    assert n % 3 == 0
    R, T, _, Tt = similar_cameras(n, seed, noise=0.05)
    D = torch.stack([torch.diag(torch.tensor(d)) for d in ((1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))]).repeat(n // 3, 1, 1)
    return R, T, D @ R, Tt


# ---- preprocessing ----------------------------------------------------------------------------------------------------------------------
PREP_CASES = ((2, 2, 1), (2, 2, 7), (3, 5, 4), (5, 3, 4), (224, 224, 224), (225, 224, 224), (224, 225, 224), (301, 533, 224), (300, 534, 224),
              (1080, 1920, 224), (3000, 4000, 224), (64, 48, 336), (300, 533, 1))
PREP_INPUTS = ("random", "checkerboard", "ramp")


def crop_box(H, W):
    c = min(H, W)
    return (H - c) // 2, (W - c) // 2, c


def prep_input(kind, H, W, seed=0):
    """uint8 [H, W, 3].  `random` and `checkerboard` carry planted values in the four corner pixels of the centre crop and the opposite
    value just outside them, so that a crop offset off by one shows in the corners too; `ramp` stays smooth (neighbours differ by <= 1)."""
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "ramp":
        tri = lambda s: np.where(s % 510 <= 255, s % 510, 510 - s % 510)      # noqa: E731
        return np.stack([tri((xx + 2 * yy) // 2), tri((2 * xx + yy) // 2 + 85), tri((xx + yy) // 2 + 170)], -1).astype(np.uint8)
    if kind == "random":
        im = np.random.default_rng(1000 + seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    else:
        im = np.repeat((((xx + yy) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
    top, left, c = crop_box(H, W)
    for k, (y, x) in enumerate(((top, left), (top, left + c - 1), (top + c - 1, left), (top + c - 1, left + c - 1))):
        v = (250, 5, 200, 60)[k]
        im[y, x] = v
        for oy, ox in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            y2, x2 = y + oy, x + ox
            inside = top <= y2 < top + c and left <= x2 < left + c
            if 0 <= y2 < H and 0 <= x2 < W and not inside:
                im[y2, x2] = 255 - v
    return im


def prep_reference(im, S, dtype):
    """torch's bilinear resize (align_corners=False, no antialiasing) of the centre crop of uint8 / 255 in `dtype` -> [3, S, S]"""
    H, W = im.shape[:2]
    top, left, c = crop_box(H, W)
    crop = torch.from_numpy(np.ascontiguousarray(im[top:top + c, left:left + c])).permute(2, 0, 1).to(dtype) / 255.0
    with one_thread():
        return F.interpolate(crop[None], size=(S, S), mode="bilinear", align_corners=False)[0]


def prep_e32(case, kind):
    H, W, S = case
    im = prep_input(kind, H, W)
    return float((prep_reference(im, S, torch.float32).double() - prep_reference(im, S, torch.float64)).abs().max())


def prep_bound(case, kind):
    return max(K_E32 * E32_PREP[(case, kind)], PREP_FLOOR)


# ---- decode -------------------------------------------------------------------------------------------------------------------------------
def decode_families(n, seed):
    """{family: pose encodings [n, 9] fp32}: quaternions of norm 1e-3 / 1 / 1e3 (unnormalised on purpose: two_s = 2 / |q|^2 does the work),
    with negative real part, within 1e-4 rad of the identity, and exact half turns (real part 0)"""
    g = torch.Generator().manual_seed(seed)
    out = {}

    def enc(q):
        e = torch.randn(n, 9, generator=g)
        e[:, 3:7] = q
        e[:, 7:9] = 0.3 * torch.randn(n, 2, generator=g)
        return e

    unit = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=1)
    out["norm 1"] = enc(unit)
    out["norm 1e-3"] = enc(unit * 1e-3)
    out["norm 1e3"] = enc(unit * 1e3)
    neg = unit.clone()
    neg[:, 0] = -neg[:, 0].abs() - 0.1
    out["negative real part"] = enc(neg)
    near = torch.cat([torch.ones(n, 1), 0.5e-4 * (2 * torch.rand(n, 3, generator=g) - 1) / math.sqrt(3.0)], dim=1)
    out["near identity"] = enc(near)
    half = torch.randn(n, 4, generator=g)
    half[:, 0] = 0.0
    out["half turn"] = enc(half)
    return out


def decode_oracle(enc, dtype, bias=1.8, fmin=0.1, fmax=20.0):
    with one_thread():
        d = O.pose_encoding_to_camera(enc.to(dtype), bias, fmin, fmax)
    return d["R"].double(), d["T"], d["focal_length"].double()


def decode_errs(R, f, R64, f64):
    """(largest absolute error of a rotation entry, largest relative error of a focal length)"""
    return float((R.double() - R64).abs().max()), float(((f.double() - f64).abs() / f64.abs()).max())


def ulp_distance(a, b):
    """elementwise distance of two fp32 arrays in units of the spacing of the larger magnitude"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


if __name__ == "__main__":          # python tests/metrics_checks.py: the tables above, from this CPU
    gold = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_edges.npz")))
    for name, tab in zip(("E32_ROT", "E32_TRA", "E32_ARE"), measure_angle_e32(gold)):
        print(name, "= {" + ", ".join(f"{k!r}: {v:.2e}" for k, v in tab.items()) + "}")
    dr, df = {}, 0.0
    for n in (1, 257, 100000):
        for fam, e in decode_families(n, 500 + n).items():
            R64, _, f64 = decode_oracle(e, torch.float64)
            R32, _, f32 = decode_oracle(e, torch.float32)
            a, b = decode_errs(R32, f32, R64, f64)
            dr[fam], df = max(dr.get(fam, 0.0), a), max(df, b)
    print("E32_DECODE_R = {" + ", ".join(f"{k!r}: {v:.2e}" for k, v in dr.items()) + "}")
    print(f"E32_DECODE_F = {df:.2e}")
    print("E32_PREP = {")
    for case in PREP_CASES:
        print("    " + " ".join(f"({case}, {k!r}): {prep_e32(case, k):.2e}," for k in PREP_INPUTS))
    print("}")
