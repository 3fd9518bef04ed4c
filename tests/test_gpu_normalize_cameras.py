"""GPU (-m gpu): pd_normalize_cameras through posediffusion_amd.normalize_cameras_batch against the yardstick of tests/normalize_checks.py.

Accuracy: per output group (R, T, p_intersect, scale, dist, foot points) and per sequence, the kernel's distance from the fp64 yardstick
(evaluated on the fp32 inputs upcast) is at most 4 x the fp32 yardstick's own distance from it, or 4 fp32 ulps of the group's magnitude
where that is larger (normalize_checks.group_ratio <= 1).  Status is 0 on every ring scene.  The worst ratio per group is printed when
the module is done, and written to $PD_PARITY_DIR/normalize_parity.txt where that variable names a directory (kept as
profiles/normalize_parity.txt).  Everything that must not depend on the launch is bitwise."""
import functools
import os

import pytest
import torch

import normalize_checks as NC
from conftest import load_golden
from posediffusion_amd import _lib, cameras

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    yield
    if not _WORST:
        return
    text = ("pd_normalize_cameras against tests/normalize_checks.py: worst over the sequences of a test family of\n"
            "  (kernel - fp64 yardstick) / max(4 x (fp32 yardstick - fp64 yardstick), 4 fp32 ulps), per output group; the bound is 1\n")
    for fam in sorted(_WORST):
        text += f"{fam:28s} " + "  ".join(f"{g} {v:.3f}" for g, v in _WORST[fam].items()) + "\n"
    print(text)
    out = os.environ.get("PD_PARITY_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "normalize_parity.txt"), "w") as fh:
            fh.write(text)


def _kw(mode):
    return dict(compute_optical={0: None, 1: True, 2: False}[mode[0]], first_camera=mode[1] != 0, rotation_only=mode[1] == 2,
                normalize_T=bool(mode[2]))


@functools.lru_cache(maxsize=None)
def _scene(kind, N, seed):
    """fp32 inputs of one sequence (cached: every test that uses the scene sees the same tensors and never writes to them)"""
    if kind == "ring":
        R, T = NC.ring(N, 0.3 if seed % 2 else 0.0, seed)
    elif kind == "degenerate":
        R, T = NC.exact_degenerate(N)
    elif kind == "parallel":
        R, T = NC.parallel(N)
    else:
        R, T = NC.near_parallel(N, 1e-3)
    return R.float(), T.float()


@functools.lru_cache(maxsize=None)
def _oracle(kind, N, seed, mode):
    R, T = _scene(kind, N, seed)
    return NC.normalize(R, T, mode, torch.float64), NC.normalize(R, T, mode, torch.float32)


def _batch(seqs, N_pad=None, pad_value=0.0):
    """[(R, T)] -> padded device tensors R [B, N, 3, 3], T [B, N, 3] and the counts"""
    counts = [r.shape[0] for r, _ in seqs]
    N = N_pad or max(counts)
    R = torch.full((len(seqs), N, 3, 3), pad_value)
    T = torch.full((len(seqs), N, 3), pad_value)
    for b, (r, t) in enumerate(seqs):
        R[b, :counts[b]], T[b, :counts[b]] = r, t
    return R.to(DEV), T.to(DEV), counts


def _run(seqs, mode, ragged=None, N_pad=None, pad_value=0.0, **extra):
    R, T, counts = _batch(seqs, N_pad, pad_value)
    if ragged is None:
        ragged = len(set(counts)) > 1 or N_pad is not None
    nf = torch.tensor(counts, dtype=torch.int32, device=DEV) if ragged else None
    return cameras.normalize_cameras_batch(R, T, nf, on_degenerate="status", diagnostics=True, **_kw(mode), **extra), counts


def _seq(res, b, n):
    return dict(R=res.R[b, :n].cpu(), T=res.T[b, :n].cpu(), p=res.p_intersect[b].cpu(), scale=res.scale[b].cpu(), dist=res.dist[b, :n].cpu(),
                foot=res.foot[b, :n].cpu(), axis=res.axis[b, :n].cpu())


def _check(res, b, n, oracle, family):
    ref64, ref32 = oracle
    ratios = NC.group_ratio(_seq(res, b, n), ref64, ref32)
    w = _WORST.setdefault(family, {})
    for g, v in ratios.items():
        w[g] = max(w.get(g, 0.0), v)
    print(family, b, n, {g: round(v, 3) for g, v in ratios.items()})
    assert all(v <= 1.0 for v in ratios.values()), (family, b, n, ratios)


def _same(a, b, fields=("R", "T", "pose_encoding", "p_intersect", "scale", "status", "dist", "foot", "axis")):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        if x is None and y is None:
            continue
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), f


def _focal(B, N, seed=0):
    return (torch.rand(B, N, 2, generator=torch.Generator().manual_seed(seed)) * 3 + 0.5).to(DEV)


@pytest.mark.parametrize("B", NC.BATCHES)
@pytest.mark.parametrize("N", NC.SHAPES_N)
def test_default_mode_on_rings(N, B):
    seeds = [N * 10 + b for b in range(B)]
    res, _ = _run([_scene("ring", N, s) for s in seeds], NC.DEFAULT_MODE)
    assert res.status.tolist() == [0] * B                                  # no ring sequence is excused
    for b, s in enumerate(seeds):
        _check(res, b, N, _oracle("ring", N, s, NC.DEFAULT_MODE), "rings_default_mode")
    # camera 0 is (I, 0) as far as the fp32 rotations given are orthonormal (3.6e-7 per entry of R_0^T R_0, see test_normalize_checks_cpu.py)
    assert (res.R[:, 0].cpu() - torch.eye(3)).abs().max() < 8 * NC.ULP32 and res.T[:, 0].abs().max() < 8 * NC.ULP32 * res.T.abs().max()


@pytest.mark.parametrize("mode", NC.MODES, ids=lambda m: "s%d_f%d_t%d" % m)
def test_every_mode_at_20_frames(mode):
    seeds = [201, 202, 203]
    res, _ = _run([_scene("ring", 20, s) for s in seeds], mode)
    assert res.status.tolist() == [0, 0, 0]
    for b, s in enumerate(seeds):
        _check(res, b, 20, _oracle("ring", 20, s, mode), "every_mode_n20")


@pytest.mark.parametrize("k", range(len(NC.GOLDEN_CASES)), ids=[c[0] for c in NC.GOLDEN_CASES])
def test_the_reference_made_fixture(k):
    inp, r32, r64, mode = NC.golden_case(load_golden("normalize_cameras.npz"), k)
    res, _ = _run([(inp["R"], inp["T"])], mode)
    assert res.status.tolist() == [0]
    n = inp["R"].shape[0]
    _check(res, 0, n, (NC.normalize(inp["R"], inp["T"], mode), NC.normalize(inp["R"], inp["T"], mode, torch.float32)), "reference_fixture")
    # the same bound against what the reference itself recorded: its fp64 run as the yardstick, its fp32 run as the reference's own error
    ratios = NC.group_ratio(_seq(res, 0, n), r64, r32, groups=tuple(r64))
    w = _WORST.setdefault("reference_fixture_outputs", {})
    for g, v in ratios.items():
        w[g] = max(w.get(g, 0.0), v)
    print("reference_fixture_outputs", n, {g: round(v, 3) for g, v in ratios.items()})
    assert all(v <= 1.0 for v in ratios.values()), ratios


# ---- exact equalities ----
@pytest.mark.parametrize("N", [20, 257])
def test_a_sequence_alone_and_in_the_slots_of_a_batch_of_7(N):
    me = _scene("ring", N, 77)
    F = _focal(1, N, 5)
    alone, _ = _run([me], NC.DEFAULT_MODE, focal_length=F)
    again, _ = _run([me], NC.DEFAULT_MODE, focal_length=F)
    _same(alone, again)                                                   # a second identical call
    others = [_scene("ring", N, 300 + b) for b in range(7)]
    for slot in (0, 3, 6):
        seqs = list(others)
        seqs[slot] = me
        Fb = _focal(7, N, 6)
        Fb[slot] = F[0]
        res, _ = _run(seqs, NC.DEFAULT_MODE, focal_length=Fb)
        for f in ("R", "T", "pose_encoding", "p_intersect", "scale", "status", "dist", "foot", "axis"):
            assert torch.equal(getattr(res, f)[slot], getattr(alone, f)[0]), (slot, f)


COUNTS = (20, 3, 65, 2, 257, 64, 256)


@pytest.mark.parametrize("mode", [NC.DEFAULT_MODE, (1, 1, 1), (2, 2, 1)], ids=lambda m: "s%d_f%d_t%d" % m)
def test_a_ragged_batch_and_its_padding(mode):
    seqs = [_scene("ring", n, 400 + n) for n in COUNTS]
    N = 260
    F = _focal(len(COUNTS), N, 7)
    res, _ = _run(seqs, mode, N_pad=N, focal_length=F)
    poisoned, _ = _run(seqs, mode, N_pad=N, pad_value=float("nan"), focal_length=F)
    _same(res, poisoned)                                                  # NaN in the padding rows of R and T changes no bit anywhere
    assert res.status.tolist() == [0] * len(COUNTS)
    for b, n in enumerate(COUNTS):
        alone, _ = _run([seqs[b]], mode, focal_length=F[b:b + 1, :n].contiguous())
        for f in ("R", "T", "pose_encoding", "dist", "foot", "axis"):
            assert torch.equal(getattr(res, f)[b, :n], getattr(alone, f)[0]), (b, f)
            pad = getattr(res, f)[b, n:]
            assert torch.equal(pad.view(torch.int32), torch.zeros_like(pad, dtype=torch.int32)), (b, f)      # +0, not -0
        for f in ("p_intersect", "scale", "status"):
            assert torch.equal(getattr(res, f)[b], getattr(alone, f)[0]), (b, f)
        _check(res, b, n, _oracle("ring", n, 400 + n, mode), "ragged_batch")


@pytest.mark.parametrize("mode", [NC.DEFAULT_MODE, (1, 1, 1), (0, 2, 0)], ids=lambda m: "s%d_f%d_t%d" % m)
def test_in_place_and_the_fused_encoding(mode):
    seqs = [_scene("ring", n, 500 + n) for n in (257, 20, 64)]
    R, T, counts = _batch(seqs)
    nf = torch.tensor(counts, dtype=torch.int32, device=DEV)
    F = _focal(3, 257, 8)
    kw = dict(on_degenerate="status", diagnostics=True, focal_length=F, log_focal_length_bias=0.7, min_focal_length=0.6, max_focal_length=3.0,
              **_kw(mode))
    out_of_place = cameras.normalize_cameras_batch(R, T, nf, **kw)
    Ri, Ti = R.clone(), T.clone()
    in_place = cameras.normalize_cameras_batch(Ri, Ti, nf, out=(Ri, Ti), **kw)
    assert in_place.R.data_ptr() == Ri.data_ptr() and in_place.T.data_ptr() == Ti.data_ptr()
    _same(out_of_place, in_place)
    # enc_out is bitwise pd_camera_to_pose of the returned R, T (real rows; the padding rows of the fused encoding are +0)
    enc = torch.empty(3 * 257, 9, device=DEV)
    _lib.check(_lib.load().pd_camera_to_pose(out_of_place.R.data_ptr(), out_of_place.T.data_ptr(), F.data_ptr(), 3 * 257, 0.7, 0.6, 3.0,
                                             enc.data_ptr(), torch.cuda.current_stream().cuda_stream), "pd_camera_to_pose")
    enc = enc.view(3, 257, 9)
    for b, n in enumerate(counts):
        assert torch.equal(out_of_place.pose_encoding[b, :n].view(torch.int32), enc[b, :n].view(torch.int32)), b
        assert not out_of_place.pose_encoding[b, n:].view(torch.int32).any()


# ---- branches ----
def test_the_zero_scale_branch():
    R, T = _scene("degenerate", 70, 0)
    res, _ = _run([(R, T)], (1, 0, 0))
    assert res.status.tolist() == [1]
    assert torch.equal(res.R[0].cpu(), R)                                 # R untouched
    want = (T.double() / T.double().norm().sqrt()).float()                # T / sqrt(||T||_F), rounded once
    assert torch.equal(res.T[0].cpu(), want)
    assert res.p_intersect.abs().max() == 0 and res.dist[0, 0] == 0 and float(res.scale[0]) == float(T.double().norm().sqrt().float())
    _check(res, 0, 70, _oracle("degenerate", 70, 0, (1, 0, 0)), "zero_scale_branch")
    full, _ = _run([(R, T)], (1, 1, 1))
    assert full.status.tolist() == [1]
    _check(full, 0, 70, _oracle("degenerate", 70, 0, (1, 1, 1)), "zero_scale_branch")


def test_rank_deficient_sequences_come_back_unchanged():
    par, one = _scene("parallel", 5, 0), _scene("ring", 1, 9)
    ok = _scene("ring", 5, 11)
    res, counts = _run([par, ok, one], NC.DEFAULT_MODE, focal_length=_focal(3, 5, 9))
    assert res.status.tolist() == [2, 0, 2]
    for b in (0, 2):
        n = counts[b]
        assert torch.equal(res.R[b, :n].cpu(), (par, ok, one)[b][0]) and torch.equal(res.T[b, :n].cpu(), (par, ok, one)[b][1])
        assert not res.R[b, n:].view(torch.int32).any() and res.scale[b] == 1 and res.p_intersect[b].abs().max() == 0
    _check(res, 1, 5, _oracle("ring", 5, 11, NC.DEFAULT_MODE), "beside_refused_sequences")
    # one frame is fine where no point is asked for: first_camera makes it (I, 0); normalize_T divides by nothing
    res, _ = _run([one], (2, 1, 1))
    assert res.status.tolist() == [0] and (res.R[0, 0].cpu() - torch.eye(3)).abs().max() < 8 * NC.ULP32
    assert res.T.abs().max() < 8 * NC.ULP32 * float(res.scale[0])          # T_0 - T_0 R_0^T R_0, with |T_0| / scale = scale


def test_near_parallel_axes_still_solve():
    res, _ = _run([_scene("near", 5, 0)], NC.DEFAULT_MODE)
    assert res.status.tolist() == [0]
    ref64, ref32 = _oracle("near", 5, 0, NC.DEFAULT_MODE)
    assert 900 < float(ref64["scale"]) < 1100                              # the point lies 1 / 1e-3 away
    _check(res, 0, 5, (ref64, ref32), "near_parallel_1e-3")


def test_a_nan_in_one_sequence_stays_there():
    seqs = [_scene("ring", 20, 600 + b) for b in range(3)]
    clean, _ = _run(seqs, NC.DEFAULT_MODE, focal_length=_focal(3, 20, 10))
    bad_T = seqs[1][1].clone()
    bad_T[13, 1] = float("nan")
    dirty = [seqs[0], (seqs[1][0], bad_T), seqs[2]]
    res, _ = _run(dirty, NC.DEFAULT_MODE, focal_length=_focal(3, 20, 10))
    assert res.status.tolist() == [0, 3, 0]
    for f in ("R", "T", "pose_encoding", "p_intersect", "scale", "dist", "foot", "axis"):
        for b in (0, 2):
            assert torch.equal(getattr(res, f)[b], getattr(clean, f)[b]), (f, b)
    assert torch.equal(res.R[1].cpu(), seqs[1][0]) and torch.equal(res.T[1].cpu().view(torch.int32), bad_T.view(torch.int32))
    R, T, _ = _batch(dirty)
    with pytest.raises(ValueError) as e:
        cameras.normalize_cameras_batch(R, T)                              # on_degenerate="raise" names exactly that sequence
    assert "sequence 1" in str(e.value) and "sequence 0" not in str(e.value) and "sequence 2" not in str(e.value)
    assert "non-finite" in str(e.value) and "status 3" in str(e.value)
    inf_R = seqs[1][0].clone()
    inf_R[0, 2, 2] = float("inf")
    res, _ = _run([(inf_R, seqs[1][1])], (0, 1, 0))
    assert res.status.tolist() == [3]
    zero_T, _ = _run([(seqs[0][0], seqs[0][1] * 0)], (2, 0, 0))
    assert zero_T.status.tolist() == [3] and not zero_T.T.any()
    zero_R = seqs[2][0].clone()                                           # finite, but frame 4 has no optical axis: the sums are NaN
    zero_R[4] = 0
    res, _ = _run([seqs[0], (zero_R, seqs[2][1])], NC.DEFAULT_MODE)
    assert res.status.tolist() == [0, 3] and torch.equal(res.R[1].cpu(), zero_R) and torch.equal(res.T[1].cpu(), seqs[2][1])
    assert _oracle("ring", 20, 600, NC.DEFAULT_MODE)[0]["status"] == 0 and NC.normalize(zero_R, seqs[2][1])["status"] == 3


@pytest.mark.parametrize("count", [0, 21, -3])
def test_a_bad_frame_count_is_status_4(count):
    seqs = [_scene("ring", 20, 700 + b) for b in range(3)]
    R, T, _ = _batch(seqs)
    good = cameras.normalize_cameras_batch(R, T, [20, 20, 20], on_degenerate="status", diagnostics=True, focal_length=_focal(3, 20, 11))
    nf = torch.tensor([20, count, 20], dtype=torch.int32, device=DEV)
    res = cameras.normalize_cameras_batch(R, T, nf, on_degenerate="status", diagnostics=True, focal_length=_focal(3, 20, 11))
    assert res.status.tolist() == [0, 4, 0]
    for f in ("R", "T", "pose_encoding", "p_intersect", "scale", "dist", "foot", "axis"):
        assert not getattr(res, f)[1].view(torch.int32).any(), f           # every row +0
        for b in (0, 2):
            assert torch.equal(getattr(res, f)[b], getattr(good, f)[b]), (f, b)
    with pytest.raises(ValueError, match=r"sequence 1: frame count outside \[1, N\]"):
        cameras.normalize_cameras_batch(R, T, nf)


def test_flat_input_with_batch_size_and_host_refusals():
    seqs = [_scene("ring", 20, 800 + b) for b in range(3)]
    R, T, _ = _batch(seqs)
    a = cameras.normalize_cameras_batch(R, T)
    b = cameras.normalize_cameras_batch(R.reshape(60, 3, 3), T.reshape(60, 3), batch_size=3)
    _same(a, b)
    assert a.pose_encoding is None and a.dist is None and a.R.shape == (3, 20, 3, 3) and a.status.dtype == torch.int32
    with pytest.raises(ValueError, match="does not divide"):
        cameras.normalize_cameras_batch(R.reshape(60, 3, 3), T.reshape(60, 3), batch_size=7)
    with pytest.raises(ValueError, match="one count per sequence"):
        cameras.normalize_cameras_batch(R, T, [20, 20])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cameras.normalize_cameras_batch(R.cpu(), T.cpu())
