"""GPU: the kernels that turn the sampler's output into the numbers people read -- csrc/pd_metrics.hip (relative pose errors, AUC and
accuracies, ARE, camera alignment, image preprocessing) and pd_camera_kernel / pd_finish_kernel of csrc/pd_engine.hip -- at their edges.

Every case is compared with the reference-generated fixture tests/golden/metrics_edges.npz or with the fp64 oracle on the same fp32 inputs,
never with another engine path.  The bounds are those of tests/metrics_checks.py (max(4 x e32, floor) per band of the true angle, e32 being
the CPU fp32 oracle's own distance from fp64; the cosine form where acos leaves degrees no room; the earlier tests' bounds for the exact
quantities); tests/test_metrics_checks_cpu.py shows where each comes from and that the faults these cases exist for exceed them.
Every case prints its figures (`pytest -s`: profiles/eval_kernel_parity.txt).  Through the drop-in wrappers where one exists, through the
C-ABI for what they do not expose (s_R_T_out, max_threshold limits, argument validation)."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import metrics_checks as M
from conftest import load_golden
from oracle import pd_oracle as O
from posediffusion_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PD_ERR_INVALID_ARG = -1
EDGES = load_golden("metrics_edges.npz")
REL = list(M.rel_cases(EDGES))
ARE = list(M.are_cases(EDGES))


def _dropin(name):
    import posediffusion_amd
    if posediffusion_amd.DROPIN_PATH not in sys.path:
        sys.path.insert(0, posediffusion_amd.DROPIN_PATH)
    return importlib.import_module(name)


def _cams(R, T):
    from posediffusion_amd.compat import PerspectiveCameras
    return PerspectiveCameras(focal_length=torch.ones(R.shape[0], 2), R=R, T=T)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _assert_bands(tag, *results):
    for res in results:
        print(f"{tag}: {M.describe(res)}")
    for res in results:
        assert not M.failures(res), (tag, M.describe(M.failures(res)))


# ---- ARE ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(ARE)), ids=[a[0].replace(" ", "_") for a in ARE])
def test_are_folds_at_90_degrees(k):
    """compute_ARE = min(e, |180 - e|): the fixture's angles (0 .. 180 about (1, 2, 3)) and random pairs, 82 % of them above 90 degrees, at
    n = 1, 127, 128, 129 (the 128-thread block and its ragged tail) and 10 000"""
    tag, Ra, Rb = ARE[k]
    got = _dropin("util.metric").compute_ARE(Ra.to(DEV), Rb.to(DEV))
    ref = M.are_oracle(Ra, Rb, np.float64)
    assert got.shape == ref.shape and not M.mask_errs(got, ref)
    above = int((M.unfolded_are(Ra, Rb) > 90).sum())
    print(f"ARE {tag}: {above} of {len(ref)} pairs above 90 degrees, largest result {got.max():.4f}")
    _assert_bands(f"ARE {tag}", M.angle_errs(got, ref, M.ARE_BANDS, M.E32_ARE))
    assert np.nanmax(got) <= 90.0
    if k == 0:
        # a NaN entry and 0 * inf give NaN as np.clip does (not the clamp's -1: a folded error of 0); an infinite trace is clipped to -1:
        # 180 degrees folded to 0, within two fp32 ulps of the 180 it is formed at (and inside its band's cosine bound above)
        assert np.isnan(got).tolist() == [False] * 20 + [True, False, True] and not M.mask_errs(got, EDGES["are_deg"])
        assert 0.0 <= got[21] <= 2 * np.spacing(np.float32(180.0)) and ref[21] == 0.0
        assert int((M.unfolded_are(Ra[:20], Rb[:20]) > 90).sum()) == 9 and abs(got[7] - 60.0) < 1e-3 and abs(got[17] - 60.0) < 1e-3       # 120 degrees reads 60, as the reference has it
        fix = M.angle_errs(got, EDGES["are_deg"].astype(np.float64), M.ARE_BANDS, {b: 2 * v for b, v in M.E32_ARE.items()})
        assert not M.failures(fix), M.describe(fix)           # the recorded fp32 values themselves: one more e32 away at most


# ---- relative pose errors -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(REL)), ids=[c[0].replace(" ", "_").replace(",", "") for c in REL])
def test_relative_pose_errors(k):
    """camera_to_rel_deg on every fixture case (identical cameras, turns of 1e-3 .. 180 degrees through both extrapolated ends of the acos,
    zero / parallel / anti-parallel / orthogonal relative translations, the 1e6 default), on random cameras from N = 2 to launches of several
    128-thread blocks with a ragged tail, and with translations scaled by 1e-6 / 1e6 (the + 1e-15 of the norms)"""
    tag, Rp, Tp, Rg, Tg, B, N = REL[k]
    r, t = _dropin("util.metric").camera_to_rel_deg(_cams(Rp, Tp), _cams(Rg, Tg), torch.device(DEV), B)
    r, t = r.cpu().numpy(), t.cpu().numpy()
    r64, t64 = M.rel_oracle(Rp, Tp, Rg, Tg, B, torch.float64)
    assert r.shape == r64.shape == (B * N * (N - 1) // 2,)
    assert not M.mask_errs(r, r64) and not M.mask_errs(t, t64), (tag, M.mask_errs(r, r64), M.mask_errs(t, t64))
    _assert_bands(tag, M.angle_errs(r, r64, M.ROT_BANDS, M.E32_ROT, N), M.angle_errs(t, t64, M.TRA_BANDS, M.E32_TRA, N))
    if tag == "fixture trans":
        # non-finite translations: the 1e6 rad default, and a NaN rotation error where the second camera of the pair carries it
        assert np.all(t[9:] > M.DEFAULT_MIN) and np.all(t[:9] <= 90.0) and np.isnan(r).tolist() == [False] * 9 + [True, False, True]
        # zero on either side or on both, orthogonal: 90 degrees as the reference gives, to the spacing of an fp32 number there
        assert np.abs(t[[0, 1, 2, 5]].astype(np.float64) - 90.0).max() <= 2 * np.spacing(np.float32(90.0))
    if tag == "fixture same":
        assert np.all((r > 0.40) & (r < 0.41))                 # identical cameras: the extrapolated acos gives 0.405 degrees, not 0


def test_pair_order_is_torch_combinations():
    """prediction == ground truth except camera 1 of sequence 1 (turned by 10 degrees) and camera 3 of it (by 20 about another axis): the
    pairs holding one of them read 10 or 20, every other pair 0.405, and ONLY the pair (1, 3) reads something else -- at the index
    torch.combinations gives it.  The drop-in rotation_angle on explicit relative rotations agrees with the same oracle."""
    axis_rotation = O.axis_rotation
    Mm = _dropin("util.metric")
    B, N = 3, 5
    _, _, Rg, Tg = M.random_cameras(B, N, 77)
    Rp = Rg.clone()
    Rp[N + 1] = (Rg[N + 1].double() @ axis_rotation((1.0, 2.0, 3.0), 10.0)).float()
    Rp[N + 3] = (Rg[N + 3].double() @ axis_rotation((-2.0, 0.5, 1.0), 20.0)).float()
    r, t = Mm.camera_to_rel_deg(_cams(Rp, Tg), _cams(Rg, Tg), torch.device(DEV), B)
    r = r.cpu().numpy()
    r64, t64 = M.rel_oracle(Rp, Tg, Rg, Tg, B, torch.float64)
    _assert_bands("pair order", M.angle_errs(r, r64, M.ROT_BANDS, M.E32_ROT, N), M.angle_errs(t.cpu().numpy(), t64, M.TRA_BANDS, M.E32_TRA, N))
    odd = [k for k in range(len(r)) if min(abs(r[k] - 0.405), abs(r[k] - 10.0), abs(r[k] - 20.0)) > 0.05]
    combos = torch.combinations(torch.arange(N), 2).tolist()
    assert odd == [10 + combos.index([1, 3])] and M.pair_of(odd[0], N) == (1, 1, 3), (odd, r)
    touched = sorted(10 + k for k, (i, j) in enumerate(combos) if i in (1, 3) or j in (1, 3))
    assert sorted(k for k in range(len(r)) if r[k] > 1.0) == touched
    ra = Mm.rotation_angle(Rg[:N].to(DEV), Rp[N:2 * N].to(DEV)).cpu().numpy()
    ref = (O.so3_relative_angle(Rg[:N].double(), Rp[N:2 * N].double()) * 180.0 / np.pi).numpy()
    _assert_bands("rotation_angle", M.angle_errs(ra, ref, M.ROT_BANDS, M.E32_ROT))
    assert Mm.rotation_angle(Rg[:4].to(DEV), Rp[N:N + 4].to(DEV), batch_size=2).shape == (2, 2)


# ---- summary ----------------------------------------------------------------------------------------------------------------------------------
def _summary(r, t, max_threshold):
    """pd_metrics_summary through the C-ABI -> (return code, out7 as fp64 numpy)"""
    rd, td = torch.as_tensor(r, dtype=torch.float32).to(DEV).contiguous(), torch.as_tensor(t, dtype=torch.float32).to(DEV).contiguous()
    out = torch.full((7,), float("nan"), device=DEV)
    rc = _lib.load().pd_metrics_summary(rd.data_ptr(), td.data_ptr(), rd.numel(), int(max_threshold), out.data_ptr(), _stream())
    return rc, out.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("k", range(4), ids=["max_threshold_1", "max_threshold_5", "max_threshold_30", "max_threshold_64"])
def test_summary_on_every_bin_edge_and_threshold(k):
    """the fixture's 80 pairs: 0, -0.0, every integer 1 .. 30, both neighbours of 1 / 5 / 15 / 30 / 64, the right-closed last bin, negative,
    1e6, the 1e6 rad default, inf, and NaN in r only, in t only and in both (in no bin and below no threshold, but counted in n)"""
    Mm = _dropin("util.metric")
    r, t, mt = EDGES["auc_r"], EDGES["auc_t"], int(EDGES["auc_thresholds"][k])
    exp = [float(EDGES["auc"][k])] + [float(v) for v in EDGES["racc"]] + [float(v) for v in EDGES["tacc"]]
    rc, got = _summary(r, t, mt)
    print(f"summary max_threshold {mt}: got {got.tolist()}, reference {exp}")
    assert rc == 0 and not M.summary_errs(got, exp), M.summary_errs(got, exp)
    assert not M.summary_errs(got, M.summary_expected(r, t, mt))
    s = Mm.metrics_summary(torch.from_numpy(r).to(DEV), torch.from_numpy(t).to(DEV), mt)
    assert list(s) == [f"Auc_{mt}", "Racc_5", "Racc_15", "Racc_30", "Tacc_5", "Tacc_15", "Tacc_30"] and not M.summary_errs(list(s.values()), exp)
    assert abs(Mm.calculate_auc_np(r, t, max_threshold=mt) - exp[0]) <= M.AUC_TOL
    finite = ~(np.isnan(r) | np.isnan(t))                       # without the NaN pairs the AUC is another number: they are dropped, not binned
    assert abs(M.summary_expected(r[finite], t[finite], mt)[0] - exp[0]) > 100 * M.AUC_TOL


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100000])
def test_summary_sizes_around_the_block(n):
    """prefixes of four repeats of the edge array around the 256-thread block, and 1 250 whole repeats of it (the expected values stay put)"""
    r, t = EDGES["auc_r"], EDGES["auc_t"]
    reps = -(-max(n, 320) // len(r))
    R, T = np.tile(r, reps)[:n], np.tile(t, reps)[:n]
    for mt in (30, 64) if n == 100000 else (30,):
        exp = M.summary_expected(R, T, mt)
        rc, got = _summary(R, T, mt)
        print(f"summary n {n} max_threshold {mt}: got {got.tolist()}, expected {exp}")
        assert rc == 0 and not M.summary_errs(got, exp), M.summary_errs(got, exp)
        if n == 100000:
            assert np.allclose(exp, M.summary_expected(r, t, mt), rtol=0, atol=1e-12)


def test_summary_rejects_max_threshold_outside_1_to_64():
    r, t = EDGES["auc_r"], EDGES["auc_t"]
    for mt in (0, 65, -1):
        rc, got = _summary(r, t, mt)
        assert rc == PD_ERR_INVALID_ARG and np.isnan(got).all() and "max_threshold" in _lib.last_error()
    assert _summary(r, t, 64)[0] == 0 and _summary(r, t, 1)[0] == 0
    with pytest.raises(RuntimeError):
        _dropin("util.metric").metrics_summary(torch.from_numpy(r).to(DEV), torch.from_numpy(t).to(DEV), 65)


# ---- alignment --------------------------------------------------------------------------------------------------------------------------------
def _align(Rs, Ts, Rt, Tt, estimate_scale, eps, want_srt=True):
    d = [x.to(DEV).float().contiguous() for x in (Rs, Ts, Rt, Tt)]
    Ro, To = torch.full_like(d[0], float("nan")), torch.full_like(d[1], float("nan"))
    srt = torch.full((13,), float("nan"), device=DEV)
    rc = _lib.load().pd_align_cameras(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), Rs.shape[0], int(estimate_scale),
                                      C.c_float(eps), Ro.data_ptr(), To.data_ptr(), srt.data_ptr() if want_srt else None, _stream())
    assert rc == 0, _lib.last_error()
    return Ro.cpu().double(), To.cpu().double(), srt.cpu().double()


ALIGN_CASES = {
    "n20_scale_on": (lambda: M.similar_cameras(20, 30, noise=0.05), 1, 1e-9),
    "n20_scale_off": (lambda: M.similar_cameras(20, 30, noise=0.05), 0, 1e-9),
    "n1": (lambda: M.similar_cameras(1, 11), 1, 1e-9),
    "n2": (lambda: M.similar_cameras(2, 12), 1, 1e-9),
    "n2_scale_off": (lambda: M.similar_cameras(2, 12), 0, 1e-9),
    "n1000": (lambda: M.similar_cameras(1000, 1010, noise=0.05), 1, 1e-9),
    "scale_1e-3": (lambda: M.similar_cameras(20, 30, scale=1e-3, noise=0.05), 1, 1e-9),
    "scale_1e3": (lambda: M.similar_cameras(20, 30, scale=1e3, noise=0.05), 1, 1e-9),
    "same_A_eps_1e-9": (lambda: M.same_A_cameras(20, 8), 1, 1e-9),
    "same_A_eps_1e-2": (lambda: M.same_A_cameras(20, 8), 1, 1e-2),
    "negative_determinant": (lambda: M.negative_det_cameras(21, 7), 1, 1e-9),
}


@pytest.mark.parametrize("name", list(ALIGN_CASES))
def test_alignment_vs_fp64_oracle(name):
    """pd_align_cameras against O.corresponding_cameras_alignment in fp64 on the same fp32 inputs: scale estimation on and off, n = 1 (s = 1
    by definition), 2, 20, 1 000, scales of 1e-3 and 1e3, den = 0 under two values of eps (s = num / eps), a covariance of negative
    determinant (cov = -I / 3, R_A = -I), and s_R_T_out = (s, R_A, T_A).  Only inputs whose covariance is far from singular are compared."""
    make, est, eps = ALIGN_CASES[name]
    Rs, Ts, Rt, Tt = make()
    R64, T64, s64, RA64, TA64, sv = M.align_oracle(Rs, Ts, Rt, Tt, est, eps)
    assert sv.min() / sv.max() >= M.ALIGN_MIN_COND, (name, sv)
    Ro, To, srt = _align(Rs, Ts, Rt, Tt, est, eps)
    # 5e-5 absolute as the earlier test holds inputs of this kind to; times max|T| only where the translations themselves are scaled up
    tscale = max(float(T64.abs().max()), float(TA64.abs().max())) if name == "scale_1e3" else 1.0
    assert tscale == 1.0 or tscale > 1e3
    eR, eT = float((Ro - R64).abs().max()), float((To - T64).abs().max())
    eRA, eTA, es = float((srt[1:10].reshape(3, 3) - RA64).abs().max()), float((srt[10:] - TA64).abs().max()), abs(float(srt[0]) - s64)
    print(f"alignment {name}: n {Rs.shape[0]}, singular values {sv.tolist()}, s {s64:.6g} (error {es:.2e}), R {eR:.2e}, T {eT:.2e} (scale {tscale:.3g}), "
          f"R_A {eRA:.2e}, T_A {eTA:.2e}")
    assert eR <= M.ALIGN_R_TOL and eRA <= M.ALIGN_R_TOL, (name, eR, eRA)
    assert eT <= M.ALIGN_T_TOL * tscale and eTA <= M.ALIGN_T_TOL * tscale, (name, eT, eTA, tscale)
    assert es <= M.ALIGN_R_TOL * max(1.0, abs(s64)), (name, float(srt[0]), s64)
    if not est or Rs.shape[0] == 1:
        assert float(srt[0]) == 1.0
    if name == "negative_determinant":
        assert (srt[1:10].reshape(3, 3) + torch.eye(3, dtype=torch.float64)).abs().max() < 1e-5
    if name.startswith("same_A"):
        other = M.align_oracle(Rs, Ts, Rt, Tt, est, 1e-2 if eps == 1e-9 else 1e-9)[2]
        assert abs(other / s64) > 1e6 or abs(s64 / other) > 1e6       # s = num / eps: the clamp, not den, sets it
    if name == "n20_scale_on":      # the drop-in wrapper is this call without s_R_T_out
        al = _dropin("util.metric").corresponding_cameras_alignment(_cams(Rs.to(DEV), Ts.to(DEV)), _cams(Rt.to(DEV), Tt.to(DEV)),
                                                                      estimate_scale=True, mode="extrinsics", eps=eps)
        assert torch.equal(al.R.cpu().double(), Ro) and torch.equal(al.T.cpu().double(), To)
        Ro2, To2, srt2 = _align(Rs, Ts, Rt, Tt, est, eps, want_srt=False)
        assert torch.equal(Ro2, Ro) and torch.equal(To2, To) and torch.isnan(srt2).all()


def test_alignment_of_a_rank_deficient_covariance_returns_finite_values():
    """cov = diag(0, 0, 1) (two cameras, the second target turned by half a turn about z): the SVD factors are not unique and the
    reference's own answer is arbitrary, so nothing is compared; the call must succeed and return finite values.  On an MI355X it returns
    R_A = diag(1, 1, 1) (the Jacobi sweeps find nothing to rotate; zero columns of U are replaced by unit vectors), recorded in
    profiles/eval_kernel_parity.txt."""
    Rs = torch.eye(3).expand(2, 3, 3).contiguous()
    Rt = torch.stack([torch.eye(3), torch.diag(torch.tensor([-1.0, -1.0, 1.0]))])
    Ts, Tt = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 2.0]]), torch.tensor([[0.5, 0.0, 1.0], [1.0, 1.0, 3.0]])
    sv = torch.linalg.svdvals((Rs.double() @ Rt.double().transpose(1, 2)).mean(0))
    assert sv.min() / sv.max() < M.ALIGN_MIN_COND
    Ro, To, srt = _align(Rs, Ts, Rt, Tt, 1, 1e-9)
    RA = srt[1:10].reshape(3, 3)
    print(f"alignment rank-deficient: s {float(srt[0])!r}, R_A {RA.tolist()}, T_A {srt[10:].tolist()}, |R_A R_A^T - I| {float((RA @ RA.T - torch.eye(3, dtype=torch.float64)).abs().max()):.2e}")
    assert torch.isfinite(Ro).all() and torch.isfinite(To).all() and torch.isfinite(srt).all()


# ---- preprocessing ------------------------------------------------------------------------------------------------------------------------------
def _preprocess(im, S):
    src = torch.from_numpy(im).to(DEV).contiguous()
    out = torch.full((3, S, S), float("nan"), device=DEV)
    rc = _lib.load().pd_preprocess_image(src.data_ptr(), im.shape[0], im.shape[1], int(S), out.data_ptr(), _stream())
    return rc, out.cpu()


@pytest.mark.parametrize("case", M.PREP_CASES, ids=["x".join(map(str, c)) for c in M.PREP_CASES])
def test_preprocessing_vs_fp64_bilinear(case, tmp_path):
    """pd_preprocess_image against torch's bilinear resize (align_corners=False) of the fp64 centre crop: the smallest accepted frame,
    S = 1, crop == S (exactly uint8 / 255), odd crop margins in either direction, up-sampling and large non-integer down-scaling; random
    pixels, a one-pixel 0 / 255 checkerboard (a wrong neighbour or weight moves it by order 1) with planted values at and just outside the
    crop's corners, and a smooth ramp (where the bound is the 2e-6 of the earlier test up to 300 x 534)."""
    H, W, S = case
    for kind in M.PREP_INPUTS:
        im = M.prep_input(kind, H, W)
        rc, got = _preprocess(im, S)
        assert rc == 0, _lib.last_error()
        ref = M.prep_reference(im, S, torch.float64)
        d = (got.double() - ref).abs()
        w = int(d.reshape(-1).argmax())
        err, bnd = float(d.max()), M.prep_bound(case, kind)
        print(f"preprocess {case} {kind}: error {err:.2e} at (c, y, x) = {tuple(int(v) for v in np.unravel_index(w, d.shape))}, e32 {M.E32_PREP[(case, kind)]:.2e}, bound {bnd:.2e}")
        assert torch.isfinite(got).all() and err <= bnd, (case, kind, err, bnd)
        if H == W == S:
            assert torch.equal(got, torch.from_numpy(im).permute(2, 0, 1).float() / 255.0)
    if case in ((3, 5, 4), (301, 533, 224), (64, 48, 336)):          # the drop-in wrapper gives the same frame
        from PIL import Image
        im = M.prep_input("random", H, W)
        path = os.path.join(str(tmp_path), "frame.png")
        Image.fromarray(im, "RGB").save(path)
        imgs, info = _dropin("util.load_img_folder").load_and_preprocess_images(None, S, image_paths=[path])
        top, left, c = M.crop_box(H, W)
        assert torch.equal(imgs[0].cpu(), _preprocess(im, S)[1]) and info["bboxes_xyxy"][0].tolist() == [left, top, left + c, top + c]


def test_preprocessing_rejects_one_pixel_wide_frames():
    """the reference raises on a frame whose shorter side is one pixel (load_img_folder.py: "squashed image")"""
    for H, W in ((1, 8), (8, 1), (1, 1)):
        rc, got = _preprocess(np.zeros((H, W, 3), dtype=np.uint8), 4)
        assert rc == PD_ERR_INVALID_ARG and torch.isnan(got).all(), (H, W)
    assert _preprocess(np.zeros((2, 2, 3), dtype=np.uint8), 0)[0] == PD_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        _dropin("util.load_img_folder")._bbox_and_scale(1, 8, 4)


# ---- decode and finish ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100000])
def test_pose_decode_quaternion_families(engine, n):
    """pd_pose_to_camera around the 64-thread block and at 1 563 blocks: quaternions of norm 1e-3 / 1 / 1e3 (two_s = 2 / |q|^2 normalises),
    with negative real part, within 1e-4 rad of the identity, exact half turns; R against fp64 under max(4 x e32, 1e-6), T bitwise"""
    for fam, enc in M.decode_families(n, 500 + n).items():
        R, T, f = engine.pose_to_camera(enc.to(DEV))
        R64, _, f64 = M.decode_oracle(enc, torch.float64)
        eR, ef = M.decode_errs(R.cpu(), f.cpu(), R64, f64)
        bR, bf = max(M.K_E32 * M.E32_DECODE_R[fam], M.DECODE_R_FLOOR), max(M.K_E32 * M.E32_DECODE_F, M.DECODE_F_FLOOR)
        w = int((R.cpu().double() - R64).abs().reshape(n, 9).amax(1).argmax())
        print(f"decode n {n} {fam}: R {eR:.2e} at camera {w} (e32 {M.E32_DECODE_R[fam]:.1e}, bound {bR:.1e}), focal {ef:.2e} (bound {bf:.1e})")
        assert R.shape == (n, 3, 3) and eR <= bR and ef <= bf, (n, fam, eR, bR, ef, bf)
        assert torch.equal(T.cpu(), enc[:, :3])


def test_pose_decode_zero_quaternion_and_focal_clamp(engine):
    enc = M.decode_families(8, 1)["norm 1"]
    enc[2, 3:7] = 0.0                                              # 2 / 0 = inf, inf * 0 = NaN: what torch's fp32 evaluation gives
    enc[3, 3:7] = torch.tensor([0.0, 0.0, 0.0, 1e-30])             # |q|^2 underflows to 0 in fp32
    enc[4, 7], enc[4, 8], enc[5, 7], enc[5, 8] = 100.0 - 1.8, -100.0 - 1.8, 98.2, -101.8          # logFL + bias = +-100
    R, T, f = engine.pose_to_camera(enc.to(DEV))
    ref = O.pose_encoding_to_camera(enc)
    assert torch.equal(torch.isfinite(R.cpu()), torch.isfinite(ref["R"])) and torch.equal(torch.isnan(R.cpu()), torch.isnan(ref["R"]))
    assert not torch.isfinite(R[2].cpu()).any() and torch.isfinite(R[[0, 1, 4, 5, 6, 7]].cpu()).all()
    assert f[4].tolist() == [20.0, float(np.float32(0.1))] and f[5].tolist() == [20.0, float(np.float32(0.1))]
    assert torch.equal(T.cpu(), enc[:, :3])
    d = _dropin("util.camera_transform").pose_encoding_to_camera(enc.to(DEV)[None], return_dict=True, engine=engine)
    assert torch.equal(torch.nan_to_num(d["R"]), torch.nan_to_num(R)) and torch.equal(d["focal_length"], f)


@pytest.mark.parametrize("t", [0, 1, 50, 99])
def test_p_finish_vs_fp32_arithmetic(engine, seeded_diffuser, t):
    """pd_p_finish = mean + exp(0.5 logvar[t]) noise (gaussian_diffuser.py:280), in fp32: against the same expression evaluated in fp32 on the
    CPU, sigma being the correctly rounded fp32 exponential.  The compiler contracts mean + sigma * noise into one FMA, which may differ
    from the two-rounding value by one spacing of the larger operand.  MEASURED on an MI355X (profiles/eval_kernel_parity.txt): the
    allowance IS needed -- up to 10 % of the elements differ from the two-rounding value, each by exactly one spacing -- and every element
    equals the single-rounding (FMA) value bitwise; so each element must be one of the two.  With noise = NULL the mean comes back bitwise."""
    logvar = seeded_diffuser.posterior_log_variance_clipped.detach().cpu().float().numpy()
    sigma = np.float32(np.exp(np.float64(np.float32(0.5) * logvar[t])))
    for B, N in ((1, 1), (3, 7), (8, 50)):                          # 9, 189, 3 600 elements: below one 256-thread block, and 15 with a tail
        g = torch.Generator().manual_seed(40 + t)
        mean, noise = 3.0 * torch.randn(B, N, 9, generator=g), torch.randn(B, N, 9, generator=g)
        got = engine.p_finish(mean.to(DEV), noise.to(DEV), t).cpu().numpy()
        prod = sigma * noise.numpy()
        two = mean.numpy() + prod                                   # two roundings
        one = (mean.numpy().astype(np.float64) + np.float64(sigma) * noise.numpy().astype(np.float64)).astype(np.float32)      # one (FMA)
        allow = np.spacing(np.maximum(np.maximum(np.abs(mean.numpy()), np.abs(prod)), np.abs(two))).astype(np.float64)
        diff = np.abs(got.astype(np.float64) - two.astype(np.float64))
        print(f"p_finish t {t} B {B} N {N}: sigma {sigma!r}; {int((got != two).sum())} of {got.size} elements differ from the two-rounding value, "
              f"{int((got != one).sum())} from the single-rounding (FMA) value; largest difference {float((diff / allow).max()):.2f} spacings")
        assert (diff <= allow).all(), (t, B, N, float((diff / allow).max()))
        assert ((got == two) | (got == one)).all(), (t, B, N, "neither the two-rounding nor the FMA value")
        assert np.array_equal(engine.p_finish(mean.to(DEV), None, t).cpu().numpy(), mean.numpy())
