"""CPU: the helpers, references and constants of tests/metrics_checks.py -- the record of where the bounds of tests/test_gpu_eval_kernels.py
come from.  No GPU and no engine code is involved: the yardsticks are the fp32 and the fp64 oracle and torch's own bilinear resize."""
import numpy as np
import pytest
import torch

import metrics_checks as M
from oracle import pd_oracle as O


@pytest.fixture(scope="module")
def edges(golden):
    return golden["metrics_edges"]


# ---- angles -------------------------------------------------------------------------------------------------------------------------------
def test_angle_e32_constants_are_not_exceeded(edges):
    """the tables come from a CPU run over every case; the fixture, two random shapes, a scaled one and one ARE batch recomputed"""
    rot, tra, are = M.measure_angle_e32(edges, only=("fixture", "B 3 N 5", "B 2 N 50", "n 129"))
    print("e32 recomputed:", rot, tra, are)
    for got, const, bands in ((rot, M.E32_ROT, M.ROT_BANDS), (tra, M.E32_TRA, M.TRA_BANDS), (are, M.E32_ARE, M.ARE_BANDS)):
        assert set(const) == {b[0] for b in bands}
        assert set(got) == set(const), "the recomputed subset does not reach every band"
        for band, v in got.items():
            assert v <= const[band], (band, v, const[band])


def test_bands_asserted_in_degrees_stay_below_the_earlier_bounds(edges):
    for bands, const in ((M.ROT_BANDS, M.E32_ROT), (M.TRA_BANDS, M.E32_TRA), (M.ARE_BANDS, M.E32_ARE)):
        for name, _, _, mode in bands:
            if mode == "deg":
                assert M.K_E32 * const[name] < M.DEG_FIXTURE < M.DEG_RANDOM, (name, const[name])
            else:       # the cosine forms: K x e32 is a few fp32 ulps of 1, i.e. an angle of at most acos(sqrt(1 - 4 e32)) = 0.07 degrees at 0
                assert M.K_E32 * const[name] < 16 * M.ULP1, (name, const[name])
    # ... and the three cosine-form bands are the ones where degrees would not: the fp32 oracle's own error in degrees on the fixture's
    # identical cameras (translation directions coincide), on near-orthogonal random directions, and on the fixture's ARE rows near 0 / 180
    for tag, Rp, Tp, Rg, Tg, B, N in M.rel_cases(edges):
        if tag == "fixture same":
            t32, t64 = M.rel_oracle(Rp, Tp, Rg, Tg, B, torch.float32)[1], M.rel_oracle(Rp, Tp, Rg, Tg, B, torch.float64)[1]
            assert t64.max() < 0.5 and M.K_E32 * np.abs(t32 - t64).max() > M.DEG_FIXTURE
        if tag == "random B 2 N 50":          # near-orthogonal directions: 1 - (1 - d^2) is rounded at 1, acos sqrt amplifies it near 0 as well
            t32, t64 = M.rel_oracle(Rp, Tp, Rg, Tg, B, torch.float32)[1], M.rel_oracle(Rp, Tp, Rg, Tg, B, torch.float64)[1]
            near90 = t64 >= 89.0
            print("t >= 89 degrees:", near90.sum(), "pairs, fp32 oracle off by", np.abs(t32 - t64)[near90].max(), "degrees")
            assert near90.sum() >= 20 and M.K_E32 * np.abs(t32 - t64)[near90].max() > M.DEG_FIXTURE
    _, Ra, Rb = next(M.are_cases(edges))
    a32, a64 = M.are_oracle(Ra, Rb, np.float32), M.are_oracle(Ra, Rb, np.float64)
    print("ARE fixture fp32 / fp64:", a32, a64)
    assert M.K_E32 * np.nanmax(np.abs(a32 - a64)[a64 < 2]) > M.DEG_FIXTURE


def test_fp32_oracle_passes_its_own_bounds_and_faults_do_not(edges):
    for tag, Rp, Tp, Rg, Tg, B, N in M.rel_cases(edges):
        if "256" in tag or "128" in tag:
            continue
        r32, t32 = M.rel_oracle(Rp, Tp, Rg, Tg, B, torch.float32)
        r64, t64 = M.rel_oracle(Rp, Tp, Rg, Tg, B, torch.float64)
        rr, tt = M.angle_errs(r32, r64, M.ROT_BANDS, M.E32_ROT, N), M.angle_errs(t32, t64, M.TRA_BANDS, M.E32_TRA, N)
        assert not M.failures(rr) and not M.failures(tt), (tag, M.describe(rr), M.describe(tt))
        assert not M.mask_errs(t32, t64) and not M.mask_errs(r32, r64), tag
        if tag == "random B 3 N 5":
            bad = r64.copy()
            bad[13] += 4e-3                                     # far inside the 2e-2 of the earlier test
            f = M.failures(M.angle_errs(bad, r64, M.ROT_BANDS, M.E32_ROT, N))
            assert len(f) == 1 and f[0]["index"] == 13 and f[0]["pair"] == (1, 0, 4), f
            # the translation error without the square of d: acos(sqrt(|d|)) instead of acos(|d|)
            nosq = np.degrees(np.arccos(np.sqrt(np.abs(np.cos(np.radians(t64))))))
            assert M.failures(M.angle_errs(nosq, t64, M.TRA_BANDS, M.E32_TRA, N))
        if tag == "fixture same":
            bad = t64.copy()
            bad[3] = 0.1                                        # 0.1 degrees where the directions coincide: passes 2e-2? no -- and not cos^2 either
            f = M.failures(M.angle_errs(bad, t64, M.TRA_BANDS, M.E32_TRA, N))
            assert len(f) == 1 and f[0]["index"] == 3 and f[0]["mode"] == "cos2", f
            bad[3] = float("nan")
            assert M.failures(M.angle_errs(bad, t64, M.TRA_BANDS, M.E32_TRA, N)) and M.mask_errs(bad, t64)
        if tag == "fixture turn10":                             # 180 degrees: the lower extrapolation branch replaced by a plain acos(bound)
            lo = r64 >= 179.19
            assert lo.sum() >= 10
            bad = np.where(lo, np.degrees(np.arccos(-(1 - 1e-4))), r64)
            f = M.failures(M.angle_errs(bad, r64, M.ROT_BANDS, M.E32_ROT, N))
            assert len(f) == 1 and "lower" in f[0]["band"], f
    for tag, Ra, Rb in M.are_cases(edges):
        a32, a64 = M.are_oracle(Ra, Rb, np.float32), M.are_oracle(Ra, Rb, np.float64)
        res = M.angle_errs(a32, a64, M.ARE_BANDS, M.E32_ARE)
        assert not M.failures(res), (tag, M.describe(res))
        un = M.unfolded_are(Ra, Rb)
        if len(un) >= 127:
            assert 0.7 < np.mean(un > 90) < 0.92, (tag, np.mean(un > 90))     # Haar measure: 1 / 2 + 1 / pi = 82 % of random pairs are above 90 degrees
            assert M.failures(M.angle_errs(un, a64, M.ARE_BANDS, M.E32_ARE)), "the unfolded angle must fail"
    assert M.pair_of(0, 5) == (0, 0, 1) and M.pair_of(10 + 4, 5) == (1, 1, 2) and M.pair_of(9, 5) == (0, 3, 4)


def test_edge_fixture_holds_what_the_gpu_tests_rely_on(edges):
    g = edges
    assert np.nanmax(g["are_deg"]) <= 90.0 and np.isnan(g["are_deg"]).sum() == 2 and (M.unfolded_are(torch.from_numpy(g["are_Ra"][:20]), torch.from_numpy(g["are_Rb"][:20])) > 90.05).sum() == 8
    r_all = np.concatenate([M.fixture_rel_case(g, n)["r"] for n in g["rel_cases"]])
    t_all = np.concatenate([M.fixture_rel_case(g, n)["t"] for n in g["rel_cases"]])
    for _, lo, hi, _ in M.ROT_BANDS:
        assert ((r_all >= lo) & (r_all < hi)).any(), (lo, hi)
    for _, lo, hi, _ in M.TRA_BANDS:
        assert ((t_all >= lo) & (t_all < hi)).any(), (lo, hi)
    assert (t_all > M.DEFAULT_MIN).sum() == 3 and np.isnan(r_all).sum() == 2 and np.all(g["same_r"] > 0.40) and np.all(g["same_r"] < 0.41)     # identical cameras: 0.405, not 0
    tt = g["trans_t"]
    assert tt[0] == tt[1] == tt[2] == 90.0 and tt[3] < 0.05 and tt[4] < 0.05 and tt[5] == 90.0                  # zero, (anti-)parallel, orthogonal


# ---- summary --------------------------------------------------------------------------------------------------------------------------------
def test_one_misplaced_pair_moves_the_expected_summary_by_100_tolerances(edges):
    r, t = edges["auc_r"], edges["auc_t"]
    assert len(r) == 80 and 100000 % len(r) == 0
    for m, auc in zip(edges["auc_thresholds"], edges["auc"]):
        exp = M.summary_expected(r, t, int(m))
        assert abs(exp[0] - float(auc)) < 1e-12 and np.allclose(exp[1:4], edges["racc"], atol=1e-12) and np.allclose(exp[4:], edges["tacc"], atol=1e-12)
        d_auc, d_acc = M.auc_edge_sensitivity(r, t, int(m))
        print(f"max_threshold {int(m)}: one pair moves the AUC by >= {d_auc:.2e}, an accuracy by {d_acc:.2e}")
        assert d_auc >= 100 * M.AUC_TOL and d_acc >= 100 * M.ACC_TOL, (m, d_auc, d_acc)
        assert not M.summary_errs(exp, exp)
        # whole repeats leave the expected values where they are
        assert np.allclose(M.summary_expected(np.tile(r, 1250), np.tile(t, 1250), int(m)), exp, rtol=0, atol=1e-12)
    # the prefixes the GPU test takes from four repeats of the array, at max_threshold 30
    R4, T4 = np.tile(r, 4), np.tile(t, 4)
    for n in (1, 255, 256, 257):
        d_auc, d_acc = M.auc_edge_sensitivity(R4[:n], T4[:n], 30)
        assert d_auc >= 100 * M.AUC_TOL and d_acc >= 100 * M.ACC_TOL, (n, d_auc, d_acc)
    # a NaN that fmaxf would swallow (the other operand binned instead) is visible: the pairs (NaN, 0), (0, NaN), (NaN, 7.5), (7.5, NaN)
    swallowed_r, swallowed_t = np.where(np.isnan(r), t, r), np.where(np.isnan(t), r, t)
    assert abs(M.summary_expected(swallowed_r, swallowed_t, 30)[0] - float(edges["auc"][2])) > 100 * M.AUC_TOL
    wrong = M.summary_errs(M.summary_expected(swallowed_r, swallowed_t, 30), M.summary_expected(r, t, 30))
    assert wrong and wrong[0].startswith("Auc")


# ---- alignment ------------------------------------------------------------------------------------------------------------------------------
def test_alignment_inputs_are_what_they_claim():
    Rs, Ts, Rt, Tt = M.negative_det_cameras(21, 7)
    R, T, s, RA, TA, sv = M.align_oracle(Rs, Ts, Rt, Tt, True, 1e-9)
    cov = (Rs.double() @ Rt.double().transpose(1, 2)).mean(0)
    assert torch.linalg.det(cov) < -0.03 and (sv - 1 / 3).abs().max() < 1e-6 and (RA + torch.eye(3, dtype=torch.float64)).abs().max() < 1e-6
    R32, T32, (RA32, _, _) = O.corresponding_cameras_alignment(Rs, Ts, Rt, Tt)
    assert (R32.double() - R).abs().max() < M.ALIGN_R_TOL / 4 and (T32.double() - T).abs().max() < M.ALIGN_T_TOL / 4     # the fp32 oracle's own distance
    for eps in (1e-9, 1e-2):
        Rs, Ts, Rt, Tt = M.same_A_cameras(20, 8)
        A = (Rs.double() @ Ts.double()[:, :, None])[:, :, 0]
        assert ((A - A.mean(0)) ** 2).mean() < 1e-12 < eps
        _, T, s, _, _, sv = M.align_oracle(Rs, Ts, Rt, Tt, True, eps)
        assert sv.min() / sv.max() >= M.ALIGN_MIN_COND and np.isfinite(s) and torch.isfinite(T).all()
    for n, scale in ((1, 0.6), (2, 0.6), (20, 1e-3), (20, 1e3), (1000, 0.6)):
        Rs, Ts, Rt, Tt = M.similar_cameras(n, 10 + n, scale=scale, noise=0.05 if n > 2 else 0.0)
        _, _, s, _, _, sv = M.align_oracle(Rs, Ts, Rt, Tt, True, 1e-9)
        assert sv.min() / sv.max() >= M.ALIGN_MIN_COND
        assert abs(s / (scale if n > 1 else 1.0) - 1) < 0.1, (n, s)


# ---- preprocessing --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.PREP_CASES)
def test_preprocessing_e32_table_is_not_exceeded(case):
    H, W, S = case
    for kind in M.PREP_INPUTS:
        e = M.prep_e32(case, kind)
        assert e <= M.E32_PREP[(case, kind)], (case, kind, e)
        if kind == "ramp":
            im = M.prep_input(kind, H, W).astype(np.int64)
            assert np.abs(np.diff(im, axis=0)).max(initial=0) <= 1 and np.abs(np.diff(im, axis=1)).max(initial=0) <= 1
            # e32 on the ramp: below 2e-7 up to 300 x 534 (the 2e-6 floor is the bound there), 8.4e-7 at 1080 x 1920, 1.5e-6 at 3000 x 4000
            assert M.prep_bound(case, kind) == M.PREP_FLOOR or H >= 1080 and M.prep_bound(case, kind) < 7e-6
        else:
            # a wrong neighbour or weight moves a 0 / 255 checkerboard output by order 1: every bound is far below that
            assert M.prep_bound(case, kind) < 2e-3
    if case == (224, 224, 224):
        im = M.prep_input("random", H, W)
        assert torch.equal(M.prep_reference(im, S, torch.float64), torch.from_numpy(im).permute(2, 0, 1).double() / 255.0)
    if H != W:                          # a crop shifted by one pixel is far outside the bound on every input
        for kind in M.PREP_INPUTS:
            if S == 1 and kind == "checkerboard":
                continue                # the one output pixel is the mean of four neighbours: 127.5 wherever the crop starts
            im = M.prep_input(kind, H, W)
            shifted = np.roll(im, 1, axis=0 if H > W else 1)
            d = (M.prep_reference(shifted, S, torch.float64) - M.prep_reference(im, S, torch.float64)).abs().max().item()
            assert d > 100 * M.prep_bound(case, kind), (case, kind, d)


# ---- decode -----------------------------------------------------------------------------------------------------------------------------------
def test_decode_e32_constants_are_not_exceeded_and_families_are_what_they_claim():
    fams = M.decode_families(257, 500 + 257)
    assert set(fams) == set(M.E32_DECODE_R)
    for fam, e in fams.items():
        R64, T, f64 = M.decode_oracle(e, torch.float64)
        R32, T32, f32 = M.decode_oracle(e, torch.float32)
        a, b = M.decode_errs(R32, f32, R64, f64)
        print(f"{fam}: fp32 oracle vs fp64: R {a:.2e}, focal {b:.2e}")
        assert a <= M.E32_DECODE_R[fam] and b <= M.E32_DECODE_F and torch.equal(T32, e[:, :3])
        assert (R64 @ R64.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-6       # a rotation whatever the norm
        q = e[:, 3:7].double()
        if fam.startswith("norm"):
            assert (q.norm(dim=1) / float(fam.split()[1]) - 1).abs().max() < 1e-5
        if fam == "negative real part":
            assert (q[:, 0] < 0).all()
        if fam == "near identity":
            assert (2 * torch.atan2(q[:, 1:].norm(dim=1), q[:, 0])).max() < 1e-4
        if fam == "half turn":
            assert (R64.diagonal(dim1=1, dim2=2).sum(1) + 1).abs().max() < 1e-6                          # trace -1
        # two_s = 2 / sqrt(|q|^2) is only right at norm 1
        eye = torch.eye(3, dtype=torch.float64)
        wrong = eye + (R64 - eye) * q.norm(dim=1)[:, None, None]
        if fam in ("norm 1e-3", "norm 1e3"):
            assert (wrong - R64).abs().max() > 0.1
    assert M.ulp_distance(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1.0
