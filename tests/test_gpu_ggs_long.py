"""GPU (-m gpu): geometry-guided sampling for sequences of 65 .. 256 frames -- the engine option PD_OPT_GGS_MAX_FRAMES and pd_ggs_long_kernel
(csrc/pd_ggs_kernels.h), on an engine of max_B = 4, max_N = 256 with the option at 256.

  1. 65 / 129 / 256 frames (8 / 4 / 3 matches per pair, all one-order pairs) against the fp64 oracle with the rules of tests/ggs_checks.py:
     the plan (long kernel, k = 256), loss + gradient, 3 iterations of GGS_optimize, one shortened geometry_guided_sampling; at 65 frames
     also 3 and 17 workgroups per sequence, bitwise the 256-workgroup result.
  2. 100 frames with both orders of every pair (9 900 pairs: 198 incidence rows per frame, more than the two-hop kernel's 128-row window).
  3. PD_GGS_CFG_LONG_FRAMES at 33 and 64 frames: bitwise the two-hop kernel.
  4. A ragged batch above 64 frames: counts (100, 40, 8) in one padded launch.
  5. Guided sampling at 65 frames: hipGraph replay equals eager launches; the drop-in with ggs_max_frames = 128, and its refusal at the default.
  6. Limits and refusals, each followed by a working GGS call at 20 frames on the same engine.

What "bitwise" covers where the workgroup count differs (1: k = 3 / 17 / 256; 4: a slot in the batch and alone): the gradient, the valid count,
the poses and the iterations stepped -- everything the update reads.  The printed loss mean is a sum of per-workgroup totals, so its last bits
follow the split of the pairs over the workgroups (as in pd_ggs2_kernel); it enters no gradient and no update, and is held to 1e-6 relative
(a few fp32 roundings of a sum of positive terms) there.  With equal workgroup counts (3) it is bitwise too.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ggs_checks import check_loss_grad, check_steps, oracle_guide, oracle_optimize
from oracle import pd_oracle as O
from posediffusion_amd import _lib, synth
from posediffusion_amd.engine import PoseEngine, make_ggs_cfg
from posediffusion_amd.host import denoiser_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LONG = _lib.PD_GGS_CFG_LONG_FRAMES
OPT = _lib.PD_OPT_GGS_MAX_FRAMES
GUIDE_CFG = dict(synth.GGS_CFG, iter_num=2)


def _engine(diff, max_B, max_N, **kw):
    return PoseEngine(denoiser_state(diff.model), {k: v for k, v in diff.named_buffers(recurse=False)}, device=torch.device(DEV),
                      max_B=max_B, max_N=max_N, **kw)


@pytest.fixture(scope="module")
def eng(seeded_diffuser):
    e = _engine(seeded_diffuser.to(torch.device(DEV)), 4, 256, ggs_max_frames=256)
    assert e.ggs_max_frames == 256
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _scene(N, per_pair, ordered=False, seed=None):
    seed = 800 + N if seed is None else seed
    enc = synth.make_cameras(N, seed=seed)
    md = synth.make_matches(enc, 224, 224, per_pair=per_pair, seed=seed, ordered_pairs=ordered)
    pm = O.prepare_matches(md["kp1"], md["kp2"], md["i12"], md["img_shape"])
    x0 = synth.perturb_pose(enc, seed=810 + N)
    return md, pm, x0


@functools.lru_cache(maxsize=None)
def _oracle_steps(N, per_pair, ordered=False, seed=None):
    """(fp64 pose, fp32 pose) after 3 iterations of GGS_optimize (x 2: all three groups update); both step all 6."""
    _, pm, x0 = _scene(N, per_pair, ordered, seed)
    ref64, s64 = oracle_optimize(x0, pm, iter_num=3)
    ref32, s32 = oracle_optimize(x0, pm, torch.float32, iter_num=3)
    assert s64 == s32 == 6, (N, s64, s32)
    return ref64, ref32


def _upload(eng, slot, md):
    eng.set_matches(slot, md["kp1"], md["kp2"], md["i12"], md["img_shape"])


def _plan(eng, B, N, cfg, n_frames=None):
    return eng.ggs_plan(B, N, cfg, n_frames=n_frames)


def _nan0(t):
    return t.nan_to_num(-1.0)


def _loss_close(a, b, tag):
    """the loss rows of two launches with different workgroup counts: valid count bitwise, means to 1e-6 (see the module docstring)"""
    assert torch.equal(a[:, 1], b[:, 1]), (tag, a, b)
    assert torch.allclose(a[:, [0, 2]], b[:, [0, 2]], rtol=1e-6, atol=0.0), (tag, a, b)


def _check_against_fp64(eng, N, per_pair, ordered, other_wgs=(), seed=None):
    md, pm, x0 = _scene(N, per_pair, ordered, seed)
    pairs = len(np.unique(md["i12"][:, 0] * N + md["i12"][:, 1]))
    assert pairs == (N * (N - 1) if ordered else N * (N - 1) // 2)
    _upload(eng, 0, md)
    tag = f"n{N}_x{per_pair}{'_ordered' if ordered else ''}"
    p = _plan(eng, 1, N, make_ggs_cfg())
    assert p[3] == 2 and p[0] == 256, (tag, p)                      # the long kernel, 256 workgroups
    x = x0.to(DEV)
    loss, grad = eng.ggs_loss_grad(x, cfg=make_ggs_cfg())
    eng.check_async()
    eg, bg = check_loss_grad(loss[0].cpu(), grad.cpu(), x0, pm, tag)
    ref64, ref32 = _oracle_steps(N, per_pair, ordered, seed)
    out, st, _ = eng.ggs_optimize(x, cfg=make_ggs_cfg(iter_num=3))
    eng.check_async()
    assert int(st[0, 1]) == 6, (tag, st)
    es, bs = check_steps(out, x0, ref64, ref32, tag)
    print(f"\n{tag}: {pairs} pairs, plan {p}; valid {int(loss[0, 1])}; gradient {({g: f'{v:.1e}' for g, v in eg.items()})} "
          f"(bound {({g: f'{v:.1e}' for g, v in bg.items()})}); step {({g: f'{v:.1e}' for g, v in es.items()})} "
          f"(bound {({g: f'{v:.1e}' for g, v in bs.items()})})")
    g, stg = eng.ggs_guide(x, 3, make_ggs_cfg(GUIDE_CFG))
    eng.check_async()
    gd64, steps64 = oracle_guide(x0, md, GUIDE_CFG)
    gd32, _ = oracle_guide(x0, md, GUIDE_CFG, torch.float32)
    assert stg[0, :, 1].long().tolist() == steps64 == [4, 2, 2, 2, 4], (tag, stg[0, :, 1].tolist(), steps64)
    eu, bu = check_steps(g, x0, gd64, gd32, tag + "/guide")
    print(f"  guide: step {({k: f'{v:.1e}' for k, v in eu.items()})}, bound {({k: f'{v:.1e}' for k, v in bu.items()})}")
    for wgs in other_wgs:                                            # the fixed summation order does not depend on the workgroup count
        cfg = make_ggs_cfg(wgs_per_seq=wgs)
        pw = _plan(eng, 1, N, cfg)
        assert pw[3] == 2 and pw[0] == wgs, (tag, wgs, pw)
        loss_w, grad_w = eng.ggs_loss_grad(x, cfg=cfg)
        out_w, st_w, _ = eng.ggs_optimize(x, cfg=make_ggs_cfg(iter_num=3, wgs_per_seq=wgs))
        g_w, stg_w = eng.ggs_guide(x, 3, make_ggs_cfg(GUIDE_CFG, wgs_per_seq=wgs))
        eng.check_async()
        assert torch.equal(grad_w, grad) and torch.equal(out_w, out) and torch.equal(g_w, g), (tag, wgs, pw)
        assert torch.equal(st_w[:, 1:3], st[:, 1:3]) and torch.equal(stg_w[:, :, 1:3], stg[:, :, 1:3]), (tag, wgs)
        _loss_close(loss_w, loss, (tag, wgs))
        print(f"  wgs_per_seq = {wgs}: plan {pw}; loss row bitwise: {torch.equal(loss_w, loss)}")


# ------------------------------------------------------------------------------------------------ 1. against fp64
@pytest.mark.parametrize("N,per_pair", [(65, 8), (129, 4), (256, 3)])
def test_long_kernel_vs_fp64(eng, N, per_pair):
    _check_against_fp64(eng, N, per_pair, False, other_wgs=(3, 17) if N == 65 else ())


# ------------------------------------------------------------------------------------------------ 2. both orders of every pair
def test_both_orders_of_every_pair_at_100_frames(eng):
    """9 900 pairs of 2 matches: a frame has 198 incidence rows (the fp64 and fp32 oracles step all 6 iterations at 2 per pair).

    Scene seed 901, chosen from the ORACLE's values alone: at the start point the Sampson distances nearest the threshold of 10 are 9.9971
    and 10.0016 in fp64, and the fp64 and fp32 oracles count the same 12 391 valid matches.  (Seed 800 + N = 900 holds a match at
    10.0000124 in fp64 -- 1.2e-6 from the threshold, valid in the fp32 oracle -- followed by one at 10.0022: ggs_checks.sampson_max_for
    cuts at the midpoint of those two, 1.1e-4 from the threshold, outside its 1e-4 band whatever code counts the valid matches in fp32.)"""
    _check_against_fp64(eng, 100, 2, True, seed=901)


# ------------------------------------------------------------------------------------------------ 3. bitwise the two-hop kernel
@pytest.mark.parametrize("N,per_pair,seed", [(33, 16, 833), (64, 8, 864)])       # n33_x16, n64_x8 of test_gpu_frame_range.py
@pytest.mark.parametrize("wgs", [0, 17])
def test_long_frames_flag_is_bitwise_the_two_hop_kernel(eng, N, per_pair, seed, wgs):
    md, _, x0 = _scene(N, per_pair, False, seed)
    _upload(eng, 0, md)
    x = x0.to(DEV)
    res = {}
    for flag in (0, LONG):
        p = _plan(eng, 1, N, make_ggs_cfg(wgs_per_seq=wgs, reserved=flag))
        assert p[3] == (2 if flag else 1), (N, wgs, flag, p)
        loss, grad = eng.ggs_loss_grad(x, cfg=make_ggs_cfg(wgs_per_seq=wgs, reserved=flag))
        out, st, _ = eng.ggs_optimize(x, cfg=make_ggs_cfg(iter_num=3, wgs_per_seq=wgs, reserved=flag))
        g, stg = eng.ggs_guide(x, 3, make_ggs_cfg(GUIDE_CFG, wgs_per_seq=wgs, reserved=flag))
        eng.check_async()
        assert int(st[0, 1]) == 6 and stg[0, :, 1].long().tolist() == [4, 2, 2, 2, 4], (N, wgs, flag, st, stg)
        res[flag] = (p[0], loss, grad, out, _nan0(st), g, _nan0(stg))
    assert res[0][0] == res[LONG][0], (res[0][0], res[LONG][0])             # the same workgroup count
    for a, b in zip(res[0][1:], res[LONG][1:]):
        assert torch.equal(a, b), (N, wgs)


# ------------------------------------------------------------------------------------------------ 4. a ragged batch above 64 frames
RAGGED = ((100, 3), (40, 8), (8, 60))          # (frames, matches per pair) of slots 0, 1, 2; padded to 100 frames


def test_ragged_batch_above_64_frames(eng):
    B, NP = len(RAGGED), 100
    counts = [n for n, _ in RAGGED]
    scenes = [_scene(n, pp) for n, pp in RAGGED]
    x = torch.zeros(B, NP, 9)
    for b, (n, _) in enumerate(RAGGED):
        x[b, :n] = scenes[b][2][0]
    # every sequence alone, at its own N, on the long kernel (the flag where N <= 64)
    alone = []
    for b, (n, pp) in enumerate(RAGGED):
        _upload(eng, 0, scenes[b][0])
        flag = LONG if n <= 64 else 0
        xb = x[b:b + 1, :n].to(DEV)
        assert _plan(eng, 1, n, make_ggs_cfg(reserved=flag))[3] == 2
        loss, grad = eng.ggs_loss_grad(xb, cfg=make_ggs_cfg(reserved=flag))
        out, st, _ = eng.ggs_optimize(xb, cfg=make_ggs_cfg(iter_num=3, reserved=flag))
        eng.check_async()
        alone.append((loss, grad, out, st))
        # ... and within the bounds of fp64
        check_loss_grad(loss[0].cpu(), grad.cpu(), scenes[b][2], scenes[b][1], f"alone{b}")
        ref64, ref32 = _oracle_steps(n, pp)
        assert int(st[0, 1]) == 6
        check_steps(out, scenes[b][2], ref64, ref32, f"alone{b}")
    for b in range(B):
        _upload(eng, b, scenes[b][0])
    p = _plan(eng, B, NP, make_ggs_cfg(), n_frames=counts)
    assert p[3] == 2, p                                                     # one launch, one family: the long kernel for all three slots
    for pad in (0.0, float("nan")):
        xp = x.clone()
        for b, n in enumerate(counts):
            xp[b, n:] = pad
        xp = xp.to(DEV)
        loss, grad = eng.ggs_loss_grad(xp, cfg=make_ggs_cfg(), n_frames=counts)
        out, st, _ = eng.ggs_optimize(xp, cfg=make_ggs_cfg(iter_num=3), n_frames=counts)
        eng.check_async()
        for b, n in enumerate(counts):
            l1, g1, o1, s1 = alone[b]
            assert torch.equal(grad[b, :n], g1[0]) and torch.equal(out[b, :n], o1[0]), (pad, b)
            assert torch.equal(st[b, 1:3], s1[0, 1:3]), (pad, b, st[b], s1)
            _loss_close(loss[b:b + 1], l1, (pad, b))
            if pad != pad:
                assert torch.isnan(out[b, n:]).all()                        # padding rows of model_mean are not touched
            else:
                assert torch.equal(out[b, n:], xp[b, n:])
    # min_matches between V / 100 and V / 40 for slot 1 (V = its valid matches): the 40-frame sequence steps every iteration -- a kernel
    # that divided by the padded frame count (100) would step none
    V = int(alone[1][0][0, 1])
    mm = (V // 100 + V // 40) // 2
    assert V / 100 < mm < V / 40, (V, mm)
    _, st_mm, _ = eng.ggs_optimize(x.to(DEV), cfg=make_ggs_cfg(iter_num=3, min_matches=mm), n_frames=counts)
    eng.check_async()
    assert int(st_mm[1, 1]) == 6, (V, mm, st_mm)


# ------------------------------------------------------------------------------------------------ 5. sampling
def geometry_guided_sampling(model_mean, t, matches_dict=None, GGS_cfg=None):      # the name host.parse_ggs_cond_fn recognises
    raise AssertionError("the engine runs GGS itself: the shipped cond_fn is never called")


def test_guided_sampling_at_65_frames_graph_eager_and_dropin(eng):
    N = 65
    md, _, _ = _scene(N, 8)
    _upload(eng, 0, md)
    z = synth.make_z(1, N, seed=31).to(DEV)
    noise = torch.randn(101, 1, N, 9, generator=torch.Generator().manual_seed(32)).to(DEV)
    cfg = dict(synth.GGS_CFG, iter_num=2)
    pose_g, proc_g, st_g = eng.sample(z, noise, 2, cfg, use_graph=True)
    pose_e, proc_e, st_e = eng.sample(z, noise, 2, cfg, use_graph=False)
    eng.check_async()
    assert torch.isfinite(pose_g).all() and torch.isfinite(proc_g).all()
    assert torch.equal(pose_g, pose_e) and torch.equal(proc_g, proc_e)
    assert torch.equal(_nan0(st_g), _nan0(st_e))
    assert not torch.equal(proc_g[-1], proc_g[-3])                           # the guided steps moved the poses
    # the drop-in (a diffuser of its own: the session's shared one keeps its engine)
    diff = synth.make_diffuser(seed=0).to(torch.device(DEV))
    cond_fn = functools.partial(geometry_guided_sampling, matches_dict=md, GGS_cfg=cfg)
    assert diff.ggs_max_frames == 64
    with pytest.raises(RuntimeError, match=r"limited to 64 frames.*GGS\.enable=False"):
        diff.sample((1, N, 9), z, cond_fn=cond_fn, cond_start_step=2)
    diff.ggs_max_frames = 128
    try:
        pose, process = diff.sample((1, N, 9), z, cond_fn=cond_fn, cond_start_step=2)
        assert torch.isfinite(pose).all() and torch.isfinite(process).all()
        assert diff.last_ggs_stats is not None and torch.isfinite(diff.last_ggs_stats[..., 0]).all()
    finally:
        ent = diff.model.__dict__.get("_pd_engine_cache", {}).get("e")
        if ent is not None:
            assert ent[1].ggs_max_frames == N                                # raised to min(128, the engine's max_N)
            ent[1].close()


# ------------------------------------------------------------------------------------------------ 6. limits and refusals
@pytest.fixture(scope="module")
def ref20(seeded_diffuser):
    """(matches, start pose, cfg, ggs_guide result and statistics) of 20 frames on an engine of max_N = 20"""
    enc = synth.make_cameras(20, seed=5)
    md = synth.make_matches(enc, 224, 224, per_pair=40, seed=5)
    x = torch.as_tensor(enc).reshape(1, 20, 9).float().to(DEV)
    cfg = make_ggs_cfg(dict(synth.GGS_CFG, iter_num=2))
    e = _engine(seeded_diffuser.to(torch.device(DEV)), 1, 20)
    try:
        _upload(e, 0, md)
        g, st = e.ggs_guide(x, 3, cfg)
        e.check_async()
    finally:
        e.close()
    return md, x, cfg, g, st


def _works_at_20(e, ref20):
    md, x, cfg, g_ref, st_ref = ref20
    _upload(e, 0, md)
    g, st = e.ggs_guide(x, 3, cfg)
    e.check_async()
    assert torch.equal(g, g_ref) and torch.equal(st, st_ref)


def test_option_values_and_frame_limit(seeded_diffuser, ref20):
    e = _engine(seeded_diffuser.to(torch.device(DEV)), 1, 100)
    try:
        assert e.ggs_max_frames == 64
        md65, _, x65 = _scene(65, 8)
        # a plain engine (option never set) refuses 65 frames as before
        with pytest.raises(RuntimeError, match=r"code -2.*limited to 64 frames"):
            _upload(e, 0, md65)
        with pytest.raises(RuntimeError, match=r"code -2.*limited to 64 frames"):
            e.ggs_loss_grad(x65.to(DEV), cfg=make_ggs_cfg())
        _works_at_20(e, ref20)
        for bad in (63, 257, 101):                                           # below 64, above 256, max_N + 1
            with pytest.raises(RuntimeError, match=rf"code -1.*PD_OPT_GGS_MAX_FRAMES.*max_N=100.*got {bad}"):
                e.set_option(OPT, bad)
            assert e.ggs_max_frames == 64
            _works_at_20(e, ref20)
        e.set_option(OPT, 80)
        assert e.ggs_max_frames == 80
        _upload(e, 0, md65)                                                  # 65 <= 80
        md90, _, x90 = _scene(90, 3)
        with pytest.raises(RuntimeError, match=r"code -2.*limited to 80 frames \(N=90\)"):     # N above the option's value
            _upload(e, 0, md90)
        with pytest.raises(RuntimeError, match=r"code -2.*limited to 80 frames \(N=90\)"):
            e.ggs_loss_grad(x90.to(DEV), cfg=make_ggs_cfg())
        _works_at_20(e, ref20)
        e.set_option(OPT, 64)                                                # back to the default: everything as on a fresh engine
        assert e.ggs_max_frames == 64
        with pytest.raises(RuntimeError, match=r"code -2.*limited to 64 frames"):
            _upload(e, 0, md65)
        _works_at_20(e, ref20)
    finally:
        e.close()


def test_refusals_of_the_long_kernel_leave_the_engine_usable(eng, ref20):
    N = 65
    md, _, x0 = _scene(N, 8)
    x = x0.to(DEV)
    # one frame pair of 600 matches: two work items for that pair
    extra = 600
    rng = np.random.default_rng(9)
    big = dict(md)
    big["kp1"] = np.concatenate([md["kp1"], rng.uniform(20, 200, (extra, 2))])
    big["kp2"] = np.concatenate([md["kp2"], rng.uniform(20, 200, (extra, 2))])
    big["i12"] = np.concatenate([md["i12"], np.tile(np.array([[0, 1]], dtype=md["i12"].dtype), (extra, 1))])
    _upload(eng, 0, big)
    with pytest.raises(RuntimeError, match=r"code -2.*slot 0.*more than 512 matches"):
        eng.ggs_loss_grad(x, cfg=make_ggs_cfg())
    _works_at_20(eng, ref20)
    # one workgroup per sequence
    _upload(eng, 0, md)
    with pytest.raises(RuntimeError, match=r"code -2.*wgs_per_seq=1"):
        eng.ggs_loss_grad(x, cfg=make_ggs_cfg(wgs_per_seq=1))
    with pytest.raises(RuntimeError, match=r"code -2.*wgs_per_seq=1"):
        _lib.check(eng.lib.pd_debug_ggs_plan(eng._h, 1, N, C.byref(make_ggs_cfg(wgs_per_seq=1)), (C.c_int * 8)()), "pd_debug_ggs_plan")
    _works_at_20(eng, ref20)
    # the device-side ingestion stays at 64 frames and names the way in
    kp1, kp2, i12 = (torch.as_tensor(md[k]).to(DEV) for k in ("kp1", "kp2", "i12"))
    with pytest.raises(RuntimeError, match=r"code -2.*limited to 64 frames \(n_frames=65\).*pd_ggs_set_matches"):
        eng.set_matches_async(0, kp1, kp2, i12, [0, kp1.shape[0]], md["img_shape"])
    _works_at_20(eng, ref20)
