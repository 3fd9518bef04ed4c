"""GPU (-m gpu): sequences of different frame counts in one padded batch (pd_engine_set_frame_counts, the ``n_frames=`` keyword).

Tensors stay padded [B, N, .]; sequence b has n_frames[b] frames in rows 0 .. n_frames[b]-1 of its block.  The reference of every check
is the sequence run ALONE through the fp64 oracle with its own frame count.

  1. denoiser, small path; padding rows +0; valid rows bitwise blind to NaN in the padding rows of x / z / noise
  2. attention boundaries (33, 70 and 256 frames: the 64-key tiles of pd_attn_long.h)
  3. streamed path (1 024 token rows), exact and fp16-plane modes
  4. all counts == N: bitwise the uniform call in exact mode on both sides of 1 024 rows; the fp64 rule in mode 2
  5. the shape-generic path (post-norm, no pivot)
  6. GGS per kernel family (asserted through pd_debug_ggs_plan): loss / gradient, 3 iterations, one shortened guide per slot against the
     fp64 oracle of the sequence alone; padding rows of model_mean keep a sentinel; bitwise the sequence alone where the family is the same
  7. the frame count that matters: min_matches chosen so that valid / n_b passes and valid / N does not
  8. unguided sampling: every step teacher-forced against fp64, hipGraph replay == eager, other counts through the same graph
  9. guided sampling: graph == eager, full stage counts, guided steps teacher-forced against the oracle's geometry_guided_sampling
 10. errors
 11. the drop-in GaussianDiffusion.sample(n_frames=) and SamplingPipeline.submit(n_frames=)

Tolerances are the project's own: TOL = 2e-5 per sequence for the denoiser (tests/test_gpu_frame_range.py), the fp16-plane rule
<= max(2 x exact-mode error, 2e-6), and tests/ggs_checks.py's check_loss_grad / check_steps."""
import numpy as np
import pytest
import torch

from conftest import pose_err, rel_err
from denoiser_cfgs import CONFIGS, build_dropin, fp64_copy, fp64_forward
from ggs_checks import check_loss_grad, check_steps, oracle_guide, oracle_loss_grad, oracle_optimize
from oracle import pd_oracle as O
from posediffusion_amd import _lib, synth
from posediffusion_amd.engine import PoseEngine, make_ggs_cfg
from posediffusion_amd.host import denoiser_state, draw_noise, get_engine
from posediffusion_amd.pipeline import SamplingPipeline
from posediffusion_amd.schedule import diffusion_buffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5
FUSED = _lib.PD_OPT_DENOISER_FUSED_ATTN
LANE, NOLANE = _lib.PD_GGS_CFG_LANE_ITEMS, _lib.PD_GGS_CFG_NO_LANE_ITEMS
SENTINEL = -7777.25
NAN = float("nan")


def _engine(diff, max_B, max_N):
    return PoseEngine(denoiser_state(diff.model), {k: v for k, v in diff.named_buffers(recurse=False)}, device=torch.device(DEV),
                      max_B=max_B, max_N=max_N)


@pytest.fixture(scope="module")
def small_eng(seeded_diffuser):
    """No call of this module gives it 1 024 token rows: the small-batch path."""
    eng = _engine(seeded_diffuser.to(DEV), 4, 256)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def stream_eng(seeded_diffuser):
    """max_B x max_N = 1 024 token rows: B = 32 runs the streamed path, B = 31 the small one."""
    eng = _engine(seeded_diffuser.to(DEV), 32, 32)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def ggs_eng(seeded_diffuser):
    eng = _engine(seeded_diffuser.to(DEV), 3, 40)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def sd64(oracle_weights):
    return O.cast_state_dict(oracle_weights, torch.float64)


def _inputs(B, N, seed=0):
    g = torch.Generator().manual_seed(70 * B + N + seed)
    return torch.randn(B, N, 9, generator=g), synth.make_z(B, N, seed=B + 31 + seed)


@torch.no_grad()
def _ref_seq(sd, x, z, t, b, n):
    """Denoiser.forward in the dtype of `sd` of sequence b ALONE with its n frames."""
    dt = sd["_first.weight"].dtype
    return O.denoiser_forward(sd, x[b:b + 1, :n].to(dt), torch.full((1,), t, dtype=torch.long), z[b:b + 1, :n].to(dt))[0]


def _padding_is_plus_zero(out, counts):
    """Rows at or beyond the count hold +0.0f (bit pattern 0), in every leading slice of `out` [.., B, N, 9]."""
    o = out.detach().cpu()
    for b, n in enumerate(counts):
        pad = o[..., b, n:, :]
        if pad.numel() and not bool((pad.contiguous().view(torch.int32) == 0).all()):
            return False
    return True


def _poison(t, counts, value=NAN):
    t = t.clone()
    for b, n in enumerate(counts):
        t[..., b, n:, :] = value
    return t


def _seq_errs(out, sd, x, z, t, counts, sub=None):
    return {b: rel_err(out[b, :counts[b]], _ref_seq(sd, x, z, t, b, counts[b])) for b in (range(len(counts)) if sub is None else sub)}


# ------------------------------------------------------------------------------------------------ 1. denoiser, small path
def test_ragged_denoiser_small_path_vs_fp64_and_nan_padding(small_eng, sd64):
    B, N, counts = 4, 8, (8, 5, 2, 1)
    x, z = _inputs(B, N)
    noise = torch.randn(B, N, 9, generator=torch.Generator().manual_seed(3))
    xd, zd, nd = x.to(DEV), z.to(DEV), noise.to(DEV)
    xn, zn, nn_ = _poison(xd, counts), _poison(zd, counts), _poison(nd, counts)
    for t in (99, 0):
        out = small_eng.denoise(xd, zd, t, n_frames=counts)
        errs = _seq_errs(out, sd64, x, z, t, counts)
        print(f"t = {t}: per-sequence rel. error vs fp64 (sequence alone): {({b: f'{e:.2e}' for b, e in errs.items()})}")
        assert torch.isfinite(out).all() and max(errs.values()) < TOL, errs
        assert _padding_is_plus_zero(out, counts)
        # the same call with NaN in every padding row of x and z: the valid rows do not move by a bit, the padding rows stay +0
        out_n = small_eng.denoise(xn, zn, t, n_frames=counts)
        assert torch.equal(out_n, out), (t, rel_err(out_n.nan_to_num(1e9), out))
        # p_mean / p_finish: both outputs, and the noise of the finish
        mean, x0 = small_eng.p_mean(xd, zd, t, n_frames=counts)
        mean_n, x0_n = small_eng.p_mean(xn, zn, t, n_frames=counts)
        assert torch.equal(mean, mean_n) and torch.equal(x0, x0_n)
        assert _padding_is_plus_zero(mean, counts) and _padding_is_plus_zero(x0, counts)
        nxt = small_eng.p_finish(mean, nd if t > 0 else None, t, n_frames=counts)
        nxt_n = small_eng.p_finish(_poison(mean, counts), nn_ if t > 0 else None, t, n_frames=counts)
        assert torch.equal(nxt, nxt_n) and _padding_is_plus_zero(nxt, counts) and torch.isfinite(nxt).all()
        # ... and they are the uniform arithmetic on the valid rows: mean from the fp64 model output of the sequence alone
        tb = O.diffusion_tables(dtype=torch.float64)
        for b, n in enumerate(counts):
            eps = _ref_seq(sd64, x, z, t, b, n)
            xs = x[b, :n].double()
            x0r = tb["sqrt_recip_alphas_cumprod"][t] * xs - tb["sqrt_recipm1_alphas_cumprod"][t] * eps
            mr = tb["posterior_mean_coef1"][t] * x0r + tb["posterior_mean_coef2"][t] * xs
            assert pose_err(mean[b, :n], mr) < TOL, (t, b)
    # a uniform call afterwards (the keyword cleared the counts) differs from the ragged one exactly where a sequence was shortened
    plain = small_eng.denoise(xd, zd, 99)
    ragged = small_eng.denoise(xd, zd, 99, n_frames=counts)
    assert torch.equal(plain[0], ragged[0]) and not torch.equal(plain[1, :5], ragged[1, :5])


# ------------------------------------------------------------------------------------------------ 2. attention boundaries
@pytest.mark.parametrize("B,N,counts", [(3, 33, (33, 32, 1)), (3, 70, (70, 65, 64)), (2, 256, (256, 129))])
def test_ragged_attention_boundaries_vs_fp64(small_eng, sd64, B, N, counts):
    """One key, a full tile, one past it, a last tile of 1 key (65, 129) and all four tiles, beside sequences of other lengths."""
    x, z = _inputs(B, N)
    xn, zn = _poison(x, counts).to(DEV), _poison(z, counts).to(DEV)
    for t in (99, 0):
        out = small_eng.denoise(xn, zn, t, n_frames=counts)
        errs = _seq_errs(out, sd64, x, z, t, counts)
        print(f"B = {B}, N = {N}, counts {counts}, t = {t}: {({b: f'{e:.2e}' for b, e in errs.items()})}")
        assert torch.isfinite(out).all() and max(errs.values()) < TOL, errs
        assert _padding_is_plus_zero(out, counts)


# ------------------------------------------------------------------------------------------------ 3. streamed path
def test_ragged_streamed_path_modes_0_and_2(stream_eng, sd64):
    B, N = 32, 32
    counts = tuple((32, 20, 7, 1)[b % 4] for b in range(B))
    x, z = _inputs(B, N)
    xn, zn = _poison(x, counts).to(DEV), _poison(z, counts).to(DEV)
    sub = (0, 1, 2, 3, 17, 30, 31)
    res = {}
    try:
        for t in (99, 0):
            for mode in (0, 2):
                stream_eng.set_split_precision(mode)
                outs = {}
                for fused in (0, 2):
                    stream_eng.set_option(FUSED, fused)
                    outs[fused] = stream_eng.denoise(xn, zn, t, n_frames=counts)
                assert torch.equal(outs[0], outs[2]), (t, mode)
                out = outs[0]
                assert torch.isfinite(out).all() and _padding_is_plus_zero(out, counts)
                res[(t, mode)] = max(_seq_errs(out, sd64, x, z, t, counts, sub).values())
    finally:
        stream_eng.set_option(FUSED, 1)
        stream_eng.set_split_precision(2)
    print(f"streamed, counts cycling (32, 20, 7, 1): (t, mode) -> worst per-sequence rel. error vs fp64: {({k: f'{v:.2e}' for k, v in res.items()})}")
    for t in (99, 0):
        assert res[(t, 0)] < TOL, res
        assert res[(t, 2)] <= max(2.0 * res[(t, 0)], 2e-6), res


# ------------------------------------------------------------------------------------------------ 4. all counts == N
@pytest.mark.parametrize("B", [31, 32])
def test_all_counts_equal_N_is_the_uniform_call(stream_eng, sd64, B):
    """992 rows (small path, pd_attn_kernel) and 1 024 rows (streamed, pd_attn_seq_kernel): in exact mode the key-tiled kernel with every
    length == N gives the bits of the uniform call.  Mode 2 at N <= 32 runs pd_attn_mma_kernel / the fused kernel without counts, whose sums
    are MFMA-ordered: the rule there is the error against fp64, <= max(2 x the exact mode's, 2e-6)."""
    N = 32
    x, z = _inputs(B, N, seed=5)
    xd, zd = x.to(DEV), z.to(DEV)
    counts = (N,) * B
    sub = (0, B // 2, B - 1)
    try:
        for t in (99, 0):
            stream_eng.set_split_precision(0)
            plain = stream_eng.denoise(xd, zd, t)
            full = stream_eng.denoise(xd, zd, t, n_frames=counts)
            assert torch.equal(plain, full), (B, t, rel_err(full, plain))
            e0 = max(_seq_errs(plain, sd64, x, z, t, counts, sub).values())
            stream_eng.set_split_precision(2)
            full2 = stream_eng.denoise(xd, zd, t, n_frames=counts)
            e2 = max(_seq_errs(full2, sd64, x, z, t, counts, sub).values())
            print(f"B = {B}, t = {t}: exact {e0:.2e}, mode 2 with counts == N {e2:.2e} vs fp64")
            assert e0 < TOL and e2 <= max(2.0 * e0, 2e-6), (e0, e2)
    finally:
        stream_eng.set_split_precision(2)


# ------------------------------------------------------------------------------------------------ 5. the shape-generic path
def test_ragged_generic_path_post_norm_no_pivot_vs_fp64():
    cfg = next(c for c in CONFIGS if not c.norm_first and not c.pivot)
    den = build_dropin(cfg, seed=40 + cfg.d)
    d64 = fp64_copy(den)
    eng = PoseEngine(denoiser_state(den), diffusion_buffers(), device=torch.device(DEV), max_B=3, max_N=8, num_layers=cfg.layers,
                     nhead=cfg.heads, norm_first=cfg.norm_first, pivot=cfg.pivot)
    try:
        B, N, counts = 3, 8, (8, 3, 1)
        g = torch.Generator().manual_seed(77)
        x, z = torch.randn(B, N, 9, generator=g), torch.randn(B, N, cfg.z, generator=g)
        xn, zn = _poison(x, counts).to(DEV), _poison(z, counts).to(DEV)
        for t in (99, 4):
            out = eng.denoise(xn, zn, t, n_frames=counts)
            assert torch.isfinite(out).all() and _padding_is_plus_zero(out, counts)
            assert torch.equal(out, eng.denoise(x.to(DEV), z.to(DEV), t, n_frames=counts))
            for b, n in enumerate(counts):
                e = pose_err(out[b, :n], fp64_forward(d64, x[b:b + 1, :n], torch.tensor([t]), z[b:b + 1, :n])[0])
                print(f"{cfg.name} t = {t} sequence {b} ({n} frames): {e:.2e}")
                assert e < TOL, (t, b, e)
            mean, x0 = eng.p_mean(xn, zn, t, n_frames=counts)
            assert _padding_is_plus_zero(mean, counts) and _padding_is_plus_zero(x0, counts)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 6. GGS per kernel family
_SCENES = {}


def _scene(n, per_pair, seed, band=0):
    """Cameras, matches (all pairs i < j; band > 0: only pairs at most `band` apart on the ring of frames -- a sparser match graph, which
    the lane-per-item kernel's LDS image needs at 24 frames), the oracle's view of them and the perturbed start point; built once."""
    key = (n, per_pair, seed, band)
    if key not in _SCENES:
        enc = synth.make_cameras(n, seed=seed)
        md = synth.make_matches(enc, 224, 224, per_pair=per_pair, seed=seed)
        if band:
            d = md["i12"][:, 1] - md["i12"][:, 0]
            keep = np.minimum(d, n - d) <= band
            md = dict(md, kp1=np.ascontiguousarray(md["kp1"][keep]), kp2=np.ascontiguousarray(md["kp2"][keep]),
                      i12=np.ascontiguousarray(md["i12"][keep]))
        pm = O.prepare_matches(md["kp1"], md["kp2"], md["i12"], md["img_shape"])
        _SCENES[key] = dict(n=n, md=md, pm=pm, x0=synth.perturb_pose(enc, seed=810 + n), refs={})
    return _SCENES[key]


def _oracle(sc, what, **kw):
    """fp64 and fp32 oracle results of a scene, computed once per (what, arguments)."""
    key = (what, tuple(sorted(kw.items())))
    if key not in sc["refs"]:
        if what == "optimize":
            r64, s64 = oracle_optimize(sc["x0"], sc["pm"], **kw)
            r32, s32 = oracle_optimize(sc["x0"], sc["pm"], torch.float32, **kw)
        else:
            cfg = dict(synth.GGS_CFG, **kw)
            r64, s64 = oracle_guide(sc["x0"], sc["md"], cfg)
            r32, s32 = oracle_guide(sc["x0"], sc["md"], cfg, torch.float32)
        sc["refs"][key] = (r64, s64, r32, s32)
    return sc["refs"][key]


def _family(eng, B, N, cfg, counts=None):
    p = eng.ggs_plan(B, N, cfg, n_frames=counts)
    if p[6]:
        return "lane"
    if p[3]:
        return f"two_hop_k{p[0]}"
    if p[0] > 1:
        return f"one_hop_k{p[0]}"
    return f"wave_k1_{p[4]}w"


def _upload(eng, slot, sc):
    md = sc["md"]
    eng.set_matches(slot, md["kp1"], md["kp2"], md["i12"], md["img_shape"])


def _padded(scenes, N, fill=SENTINEL):
    x = torch.full((len(scenes), N, 9), fill)
    for b, sc in enumerate(scenes):
        x[b, :sc["n"]] = sc["x0"][0]
    return x


GGS_FAMILIES = {
    # name: (N, scenes (n, per_pair, seed, band), wgs_per_seq, reserved, family expected of the ragged launch)
    "lane": (24, ((24, 30, 824, 8), (20, 30, 820, 8), (2, 200, 7, 0)), 0, LANE, "lane"),
    "wave_k1": (24, ((24, 30, 824, 0), (20, 30, 820, 0), (2, 200, 7, 0)), 1, NOLANE, "wave_k1"),
    "one_hop_k3": (24, ((24, 30, 824, 0), (20, 30, 820, 0), (2, 200, 7, 0)), 3, NOLANE, "one_hop_k3"),
    "two_hop": (40, ((40, 16, 840, 0), (33, 16, 833, 0)), 17, 0, "two_hop_k17"),
}


@pytest.mark.parametrize("case", list(GGS_FAMILIES))
def test_ragged_ggs_per_kernel_family_vs_the_sequence_alone(ggs_eng, case):
    N, specs, wgs, flags, want = GGS_FAMILIES[case]
    eng = ggs_eng
    scenes = [_scene(*s) for s in specs]
    counts = tuple(sc["n"] for sc in scenes)
    B = len(scenes)
    base = make_ggs_cfg(wgs_per_seq=wgs, reserved=flags)
    opt = make_ggs_cfg(iter_num=3, wgs_per_seq=wgs, reserved=flags)
    gcfg = dict(synth.GGS_CFG, iter_num=2)
    guide = make_ggs_cfg(gcfg, wgs_per_seq=wgs, reserved=flags)
    # every sequence ALONE: a uniform call at N = n_b from slot 0
    alone = []
    for sc in scenes:
        _upload(eng, 0, sc)
        xb = sc["x0"].to(DEV)
        fam = _family(eng, 1, sc["n"], base)
        loss, grad = eng.ggs_loss_grad(xb, cfg=base)
        out, st, _ = eng.ggs_optimize(xb, cfg=opt)
        g, gst = eng.ggs_guide(xb, 3, guide)
        eng.check_async()
        alone.append(dict(fam=fam, loss=loss[0].cpu(), grad=grad[0].cpu(), opt=out[0].cpu(), st=st[0].cpu(), guide=g[0].cpu(), gst=gst[0].cpu()))
    # the ragged launch
    for b, sc in enumerate(scenes):
        _upload(eng, b, sc)
    fam = _family(eng, B, N, base, counts)
    assert fam.startswith(want), (case, fam)
    assert _family(eng, B, N, guide, counts) == fam == _family(eng, B, N, opt, counts)
    x = _padded(scenes, N).to(DEV)
    loss, grad = eng.ggs_loss_grad(x, cfg=base, n_frames=counts)
    out, st, _ = eng.ggs_optimize(x, cfg=opt, n_frames=counts)
    g, gst = eng.ggs_guide(x, 3, guide, n_frames=counts)
    eng.check_async()
    print(f"\n{case}: N = {N}, counts {counts}: ragged launch {fam}; alone {[a['fam'] for a in alone]}")
    for b, sc in enumerate(scenes):
        n, tag = sc["n"], f"ragged/{case}/seq{b}"
        check_loss_grad(loss[b].cpu(), grad[b:b + 1, :n].cpu(), sc["x0"], sc["pm"], tag)
        r64, s64, r32, s32 = _oracle(sc, "optimize", iter_num=3)
        assert s64 == s32 == 6 and int(st[b, 1]) == 6, (tag, s64, s32, st[b].tolist())
        es, bnd = check_steps(out[b:b + 1, :n], sc["x0"], r64, r32, tag)
        g64, gs64, g32, _ = _oracle(sc, "guide", iter_num=2)
        assert gst[b, :, 1].long().tolist() == gs64 == [4, 2, 2, 2, 4], (tag, gst[b, :, 1].tolist(), gs64)
        eg, _ = check_steps(g[b:b + 1, :n], sc["x0"], g64, g32, tag + "/guide")
        print(f"  seq {b} ({n} frames): optimize step {({k: f'{v:.1e}' for k, v in es.items()})} (bound {({k: f'{v:.1e}' for k, v in bnd.items()})}), "
              f"guide step {({k: f'{v:.1e}' for k, v in eg.items()})}")
        # padding rows of model_mean: the sentinel before, the same sentinel after
        for res in (out, g):
            assert bool((res[b, n:] == SENTINEL).all()), tag
        assert bool((grad[b, n:] == 0).all()), tag                     # (ggs_loss_grad hands the kernel a zeroed gradient)
        if alone[b]["fam"] == fam:
            a = alone[b]
            assert torch.equal(loss[b].cpu(), a["loss"]) and torch.equal(grad[b, :n].cpu(), a["grad"]), tag
            assert torch.equal(out[b, :n].cpu(), a["opt"]) and torch.equal(st[b].cpu().nan_to_num(-1.0), a["st"].nan_to_num(-1.0)), tag
            assert torch.equal(g[b, :n].cpu(), a["guide"]) and torch.equal(gst[b].cpu().nan_to_num(-1.0), a["gst"].nan_to_num(-1.0)), tag
    if case == "lane":
        assert all(a["fam"] == "lane" for a in alone), alone          # (so the bitwise comparison above did run for this family)


# ------------------------------------------------------------------------------------------------ 7. the count that matters
COUNT_CASES = {
    # n_b, N, per_pair, seed: V0 (fp64 valid count at the start), min_matches = V0 // n_b - 2, and min_matches x N > V0
    "n20_of_24": (20, 24, 30, 820, 3426, 169),
    "n5_of_8": (5, 8, 200, 805, 1277, 253),
    "n33_of_40": (33, 40, 16, 833, 4703, 140),
    "n2_of_24": (2, 24, 200, 7, 171, 83),
}


@pytest.mark.parametrize("case", list(COUNT_CASES))
def test_min_matches_divides_by_the_sequences_own_frame_count(ggs_eng, case):
    """len(valid) / n_frames < min_matches (geometry_guided_sampling.py:105) with min_matches between V / N and V / n_b: the sequence alone
    steps all 6 iterations; a kernel that divided by the padded N would step none."""
    n, N, per_pair, seed, v0_want, mm_want = COUNT_CASES[case]
    sc = _scene(n, per_pair, seed)
    v0 = oracle_loss_grad(sc["x0"], sc["pm"])[0]
    mm = v0 // n - 2
    assert (v0, mm) == (v0_want, mm_want) and mm * N > v0, (v0, mm)
    r64, s64, r32, s32 = _oracle(sc, "optimize", iter_num=3, min_matches=mm)
    assert s64 == s32 == 6, (s64, s32)
    _upload(ggs_eng, 0, sc)
    x = _padded([sc], N).to(DEV)
    fams = {}
    for wgs, flags in ((0, 0), (1, NOLANE), (0, LANE)):
        cfg = make_ggs_cfg(iter_num=3, min_matches=mm, wgs_per_seq=wgs, reserved=flags)
        fams[(wgs, flags)] = _family(ggs_eng, 1, N, cfg, (n,))
        out, st, _ = ggs_eng.ggs_optimize(x, cfg=cfg, n_frames=(n,))
        ggs_eng.check_async()
        assert int(st[0, 1]) == 6, (case, wgs, flags, st[0].tolist())
        check_steps(out[:, :n], sc["x0"], r64, r32, f"ragged/count/{case}/k{wgs}/f{flags}")
        assert bool((out[0, n:] == SENTINEL).all())
    print(f"{case}: V0 = {v0}, min_matches = {mm} (x N = {mm * N}); families {fams}")


# ------------------------------------------------------------------------------------------------ 8. sampling, unguided
def _teacher_forced_unguided(process, noise, z, sd64, b, n, steps):
    """Worst per-group relative error over `steps` of sequence b: every step recomputed in fp64 FROM THE ENGINE'S OWN previous sample."""
    T = 100
    tb = O.diffusion_tables(dtype=torch.float64)
    ks = torch.as_tensor(list(steps))
    ts = T - 1 - ks
    xs = process[ks, b, :n].cpu().double()
    with torch.no_grad():
        eps = O.denoiser_forward(sd64, xs, ts, z[b:b + 1, :n].double().expand(len(ks), n, -1))
    c = lambda name: tb[name][ts].reshape(-1, 1, 1)                              # noqa: E731
    x0 = c("sqrt_recip_alphas_cumprod") * xs - c("sqrt_recipm1_alphas_cumprod") * eps
    mean = c("posterior_mean_coef1") * x0 + c("posterior_mean_coef2") * xs
    nz = noise[ks + 1, b, :n].cpu().double() * (ts > 0).reshape(-1, 1, 1)
    nxt = mean + torch.exp(0.5 * c("posterior_log_variance_clipped")) * nz
    return max(pose_err(process[k + 1, b, :n], nxt[i]) for i, k in enumerate(ks.tolist()))


def test_ragged_unguided_sampling_teacher_forced_and_graph_replay(small_eng, sd64):
    B, N = 3, 8
    z = synth.make_z(B, N, seed=41)
    noise = draw_noise((B, N, 9), 100, torch.device(DEV), generator=torch.Generator(device=DEV).manual_seed(8))
    zd = z.to(DEV)
    results = {}
    for counts in ((8, 5, 2), (3, 8, 1)):                   # the second call replays the graph the first one captured, with other counts
        zn, nn_ = _poison(zd, counts), _poison(noise, counts)
        pg, prg, _ = small_eng.sample(zn, nn_, 0, None, use_graph=True, n_frames=counts)
        pe, pre, _ = small_eng.sample(zd, noise, 0, None, use_graph=False, n_frames=counts)
        assert torch.isfinite(prg).all()
        assert torch.equal(pg, pe) and torch.equal(prg, pre) and torch.equal(pg, prg[100]), counts
        assert _padding_is_plus_zero(prg, counts) and _padding_is_plus_zero(pg, counts)        # every slice of process_out, slice 0 included
        for b, n in enumerate(counts):
            assert torch.equal(prg[0, b, :n], noise[0, b, :n])
        results[counts] = prg
    prg = results[(8, 5, 2)]
    errs = {b: _teacher_forced_unguided(prg, noise, z, sd64, b, n, range(100)) for b, n in enumerate((8, 5, 2))}
    print(f"unguided, counts (8, 5, 2): worst teacher-forced per-group rel. error over the 100 steps: {({b: f'{e:.2e}' for b, e in errs.items()})}")
    assert max(errs.values()) < TOL, errs
    errs2 = {b: _teacher_forced_unguided(results[(3, 8, 1)], noise, z, sd64, b, n, (0, 50, 99)) for b, n in enumerate((3, 8, 1))}
    assert max(errs2.values()) < TOL, errs2
    assert not torch.equal(results[(3, 8, 1)][1, 0, :3], prg[1, 0, :3])                         # the replay did take the new counts
    # uniform sampling afterwards is untouched by the ragged graphs (another graph key)
    pu, pru, _ = small_eng.sample(zd, noise, 0, None, use_graph=True)
    pv, prv, _ = small_eng.sample(zd, noise, 0, None, use_graph=False)
    assert torch.equal(pru, prv) and torch.equal(pru[:, 0], results[(8, 5, 2)][:, 0])            # (sequence 0 has all 8 frames either way)


# ------------------------------------------------------------------------------------------------ 9. sampling, guided
def test_ragged_guided_sampling_graph_equals_eager_and_teacher_forced(ggs_eng, sd64):
    """The matches of every sequence are made for the cameras the sampler itself reaches where guidance starts (the model mean at
    t = cond_start_step - 1, as bench.py does: a seeded denoiser's poses have nothing to do with a synthetic scene, and GGS on unrelated
    matches leaves at once through the min_matches test), so every stage runs all its iterations.  Those cameras are wild (an untrained
    network's) and 35 iterations on them are ill-conditioned: the fp32 oracle itself ends 0.3 .. 3 x a step away from the fp64 oracle, so
    check_steps' bound (4 x that distance) is wide here -- measured: engine 0.05 .. 2.2, bound 0.6 .. 15, per group.  The sharp per-slot
    check against the oracle is section 6 (well-conditioned scenes, 1e-5 .. 6e-3 of a step); what this test adds is the sampler around
    it: graph == eager, full stage counts, the mean that enters guidance within TOL of fp64, and the guided slice bitwise the step-level
    pd_ggs_guide on the same padded batch."""
    B, N, counts = 2, 24, (24, 20)
    z = synth.make_z(B, N, seed=43)
    noise = draw_noise((B, N, 9), 100, torch.device(DEV), 2, True, generator=torch.Generator(device=DEV).manual_seed(9))
    cfg = dict(synth.GGS_CFG, iter_num=5)
    _, pr_u, _ = ggs_eng.sample(z.to(DEV), noise, 0, None, use_graph=False, n_frames=counts)      # the unguided steps t = 99 .. 2 are the same
    mean98, _ = ggs_eng.p_mean(pr_u[98], z.to(DEV), 1, n_frames=counts)
    scenes = []
    for b, n in enumerate(counts):
        md = synth.make_epipolar_matches(mean98[b, :n].cpu().double().numpy(), 224, 224, per_pair=30, seed=900 + b)
        scenes.append(dict(n=n, md=md))
        _upload(ggs_eng, b, scenes[-1])
    zn, nn_ = _poison(z.to(DEV), counts), _poison(noise, counts)
    pg, prg, stg = ggs_eng.sample(zn, nn_, 2, cfg, use_graph=True, n_frames=counts)
    pe, pre, ste = ggs_eng.sample(z.to(DEV), noise, 2, cfg, use_graph=False, n_frames=counts)
    ggs_eng.check_async()
    assert torch.isfinite(prg).all() and torch.isfinite(pg).all()
    assert torch.equal(pg, pe) and torch.equal(prg, pre) and torch.equal(stg.nan_to_num(-1.0), ste.nan_to_num(-1.0))
    assert _padding_is_plus_zero(prg, counts) and _padding_is_plus_zero(pg, counts)
    assert stg[:, :, :, 1].long().tolist() == [[[10, 5, 5, 5, 10]] * B] * 2, stg[:, :, :, 1].tolist()      # full stage counts
    assert torch.equal(prg[:99], pr_u[:99]) and not torch.equal(prg[99, :, :2], pr_u[99, :, :2])
    # unguided steps (a sample of them) and the two guided ones, teacher-forced per sequence
    for b, n in enumerate(counts):
        e = _teacher_forced_unguided(prg, noise, z, sd64, b, n, (0, 40, 97))
        assert e < TOL, (b, e)
    for k, t in ((98, 1), (99, 0)):
        mean, _ = ggs_eng.p_mean(prg[k], z.to(DEV), t, n_frames=counts)
        g_step, _ = ggs_eng.ggs_guide(mean, t, cfg, n_frames=counts)           # the step-level API on the same padded batch: the same launches
        assert torch.equal(g_step, prg[k + 1]), t
        for b, sc in enumerate(scenes):
            n = sc["n"]
            mb = mean[b:b + 1, :n].cpu()
            e_mean = pose_err(mb, _mean64(sd64, prg[k].cpu(), z, t, b, n))
            g64, s64 = oracle_guide(mb, sc["md"], cfg)
            g32, _ = oracle_guide(mb, sc["md"], cfg, torch.float32)
            assert s64 == [10, 5, 5, 5, 10], s64
            es, bnd = check_steps(prg[k + 1, b:b + 1, :n], mb, g64, g32, f"ragged/guided/t{t}/seq{b}")
            print(f"guided step t = {t}, sequence {b} ({n} frames): mean {e_mean:.2e} vs fp64; GGS step {({g: f'{v:.1e}' for g, v in es.items()})}, "
                  f"bound {({g: f'{v:.1e}' for g, v in bnd.items()})}")
            assert e_mean < TOL, (t, b, e_mean)


@torch.no_grad()
def _mean64(sd64, x, z, t, b, n):
    tb = O.diffusion_tables(dtype=torch.float64)
    return O.p_mean_variance(sd64, tb, x[b:b + 1, :n].double(), t, z[b:b + 1, :n].double())[0]


# ------------------------------------------------------------------------------------------------ 10. errors
def test_ragged_errors_and_clearing(ggs_eng):
    eng = ggs_eng
    B, N = 2, 24
    x, z = _inputs(B, N, seed=9)
    xd, zd = x.to(DEV), z.to(DEV)
    before = eng.denoise(xd, zd, 50)
    invalid, unsupported = r"code -1", r"code -2"
    with pytest.raises(RuntimeError, match=invalid + r".*\[1, N\]"):
        eng.set_frame_counts([0, 5])                                        # count 0
    with pytest.raises(RuntimeError, match=invalid + r".*\[1, N\]"):
        eng.denoise(xd, zd, 50, n_frames=[N + 1, 5])                        # count N + 1
    with pytest.raises(RuntimeError, match=invalid + r".*\[1, N\]"):
        eng.p_finish(xd, None, 50, n_frames=[N + 1, 5])
    scenes = [_scene(24, 30, 824), _scene(20, 30, 820)]
    for b, sc in enumerate(scenes):
        _upload(eng, b, sc)
    xg = _padded(scenes, N).to(DEV)
    cfg = make_ggs_cfg(iter_num=1)
    try:
        eng.set_frame_counts([24, 20])
        with pytest.raises(RuntimeError, match=invalid + r".*B=2.*B=1"):    # B mismatch
            eng.denoise(xd[:1], zd[:1], 50)
        with pytest.raises(RuntimeError, match=invalid + r".*B=2.*B=1"):
            eng.ggs_loss_grad(xg[:1], cfg=cfg)
        with pytest.raises(RuntimeError, match=invalid + r".*B=2.*B=1"):
            eng.sample(zd[:1], torch.zeros(101, 1, N, 9, device=DEV), 0, None, use_graph=False)
        with pytest.raises(RuntimeError, match=unsupported + r".*training batches are uniform"):
            eng.p_losses(xd, zd, torch.tensor([3, 4]), xd)
        with pytest.raises(RuntimeError, match=unsupported + r".*training batches are uniform"):
            eng.denoise_t(xd, zd, torch.tensor([3, 4]))
        with pytest.raises(RuntimeError, match=invalid + r".*trace_out must be NULL"):
            eng.ggs_optimize(xg, cfg=cfg, trace=True)
        assert eng.time_kernel(0, 1, 8, reps=1) > 0.0                       # pd_time_kernel ignores the counts (B = 1 here, no error)
        eng.ggs_loss_grad(xg, cfg=cfg)                                      # the counts of the slots: accepted
        eng.set_frame_counts([24, 19])
        with pytest.raises(RuntimeError, match=invalid + r".*slot 1 matches were uploaded for 20 frames.*19"):
            eng.ggs_loss_grad(xg, cfg=cfg)
        with pytest.raises(RuntimeError, match=invalid + r".*uploaded for 20 frames"):
            eng.ggs_plan(B, N, cfg)
    finally:
        eng.set_frame_counts(None)
    eng.check_async()
    assert torch.equal(eng.denoise(xd, zd, 50), before)                     # cleared: bitwise the call made before any counts were set
    loss_u, _ = eng.ggs_loss_grad(scenes[0]["x0"].to(DEV), cfg=cfg)         # and uniform GGS (slot 0 holds 24 frames) runs again
    assert torch.isfinite(loss_u).all()


# ------------------------------------------------------------------------------------------------ 11. drop-in and pipeline
def test_dropin_sample_and_pipeline_submit_take_n_frames(seeded_diffuser):
    dev = torch.device(DEV)
    diff = seeded_diffuser.to(dev)
    B, N, counts = 2, 8, [8, 5]
    z = synth.make_z(B, N, seed=47).to(dev)
    torch.manual_seed(123)
    pose, process = diff.sample((B, N, 9), z, n_frames=counts)
    eng = get_engine(diff.model, diff, B, N)
    torch.manual_seed(123)
    noise = draw_noise((B, N, 9), 100, dev)
    p2, pr2, _ = eng.sample(z, noise, 0, None, n_frames=counts)
    assert torch.equal(pose, p2) and torch.equal(process, pr2)
    assert _padding_is_plus_zero(process, counts) and torch.isfinite(process).all()
    with pytest.raises(ValueError, match="one count in"):
        diff.sample((B, N, 9), z, n_frames=[8, 9])
    torch.cuda.synchronize()
    pipe = SamplingPipeline([eng], 1, dev)
    pend = pipe.submit(z, noise, n_frames=counts, want_process=True)
    pp, ppr, _ = pend.wait()
    assert torch.equal(pp, p2) and torch.equal(ppr, pr2)
    # the context is uniform again afterwards
    pu, _, _ = pipe.submit(z, noise, want_process=False).wait()
    assert torch.equal(pu, eng.sample(z, noise, 0, None)[0]) and not torch.equal(pu[1, :5], pp[1, :5])
