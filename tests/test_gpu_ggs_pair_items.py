"""GPU (-m gpu): GGS above 64 frames with frame pairs of more than 512 matches -- the engine option PD_OPT_GGS_LONG_PAIR_ITEMS and
pd_ggs_longm_kernel (csrc/pd_ggs_kernels.h: pd_ggs_long_kernel's scheme with a slot = a frame pair, whose wave adds the pair's work items in
item order), on one engine of max_B = 2, max_N = 65 with ggs_max_frames = 65 and the option on.  The scenes and their oracle-side figures
are those of tests/ggs_pair_items_cases.py (pinned on the CPU by tests/test_ggs_pair_items_cpu.py); tolerances are those of
tests/ggs_checks.py.

  1. 65 frames, pairs of 513 / 1 024 / 1 025 / 1 500 matches among 2 080, against the fp64 oracle: plan (kernel 3, 256 workgroups), loss +
     gradient, 3 iterations of GGS_optimize, one shortened geometry_guided_sampling.
  2. 3, 17 and 256 workgroups per sequence: bitwise the same gradient, poses, valid count and iterations (3: 696 slots in batches).
  3. Tables of single-item pairs through the new kernel are bitwise pd_ggs_long_kernel's results.
  4. A mixed launch (65 frames multi-item + 40 frames single-item): every slot bitwise what it gives alone.
  5. 33 frames under PD_GGS_CFG_LONG_FRAMES: 8 slots per workgroup, register-resident and streamed pairs side by side, against fp64.
  6. Device-built tables (hints 0 and 1 500) are bitwise the host-built ones; hint 1 024 raises the asynchronous error word.
  7. Guided sampling: hipGraph replay equals eager launches, and a re-upload of single-item tables does not replay the multi-item graph.
  8. The option's values, and the refusals of an engine with the option off, each followed by a working GGS call at 20 frames.

"Bitwise" where the workgroup count differs (2, 4) is what test_gpu_ggs_long.py's docstring says: gradient, valid count, poses, iterations;
the printed loss means are sums of per-workgroup totals and are held to the 1e-6 relative of `_loss_close` there.
"""
import functools

import pytest
import torch

import ggs_pair_items_cases as cases
from ggs_checks import check_loss_grad, check_steps, oracle_guide, oracle_optimize
from posediffusion_amd import _lib, synth
from posediffusion_amd.engine import PoseEngine, make_ggs_cfg
from posediffusion_amd.host import denoiser_state, pack_matches_ragged

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LONG = _lib.PD_GGS_CFG_LONG_FRAMES
OPT = _lib.PD_OPT_GGS_LONG_PAIR_ITEMS
GUIDE_CFG = cases.GUIDE_CFG


def _engine(diff, max_B, max_N, **kw):
    return PoseEngine(denoiser_state(diff.model), {k: v for k, v in diff.named_buffers(recurse=False)}, device=torch.device(DEV),
                      max_B=max_B, max_N=max_N, **kw)


@pytest.fixture(scope="module")
def eng(seeded_diffuser):
    e = _engine(seeded_diffuser.to(torch.device(DEV)), 2, 65, ggs_max_frames=65, ggs_long_pair_items=True)
    assert e.ggs_max_frames == 65 and e.ggs_long_pair_items is True
    yield e
    e.close()


def _upload(eng, slot, md):
    eng.set_matches(slot, md["kp1"], md["kp2"], md["i12"], md["img_shape"])


def _ingest(eng, slot, md, **hints):
    kp1, kp2, i12, off, shape, counts = pack_matches_ragged([md], pin=True)
    eng.set_matches_async(slot, kp1, kp2, i12, off, shape, n_frames=counts, **hints)


def _nan0(t):
    return t.nan_to_num(-1.0)


def _loss_close(a, b, tag):
    """the loss rows of two launches with different workgroup counts: valid count bitwise, means to 1e-6 (test_gpu_ggs_long.py)"""
    assert torch.equal(a[:, 1], b[:, 1]), (tag, a, b)
    assert torch.allclose(a[:, [0, 2]], b[:, [0, 2]], rtol=1e-6, atol=0.0), (tag, a, b)


def _run(eng, x, n_frames=None, **cfg):
    """(loss rows, gradient, poses after 3 iterations, their statistics, guided poses, their statistics) of the slots as uploaded"""
    loss, grad = eng.ggs_loss_grad(x, cfg=make_ggs_cfg(**cfg), n_frames=n_frames)
    out, st, _ = eng.ggs_optimize(x, cfg=make_ggs_cfg(iter_num=3, **cfg), n_frames=n_frames)
    g, stg = eng.ggs_guide(x, 3, make_ggs_cfg(GUIDE_CFG, **cfg), n_frames=n_frames)
    eng.check_async()
    return loss, grad, out, _nan0(st), g, _nan0(stg)


def _same_update(a, b, tag, rows=slice(None), rows_b=slice(None), frames=None):
    """gradient, poses, valid count and iterations of two runs bitwise; the loss means as _loss_close"""
    f = slice(None) if frames is None else slice(0, frames)
    for i in (1, 2, 4):
        assert torch.equal(a[i][rows][:, f], b[i][rows_b][:, f]), (tag, i)
    assert torch.equal(a[3][rows][:, 1:3], b[3][rows_b][:, 1:3]) and torch.equal(a[5][rows][:, :, 1:3], b[5][rows_b][:, :, 1:3]), tag
    _loss_close(a[0][rows], b[0][rows_b], tag)


@functools.lru_cache(maxsize=None)
def _oracle65():
    """the fp64 / fp32 oracle's 3 iterations and shortened guide of scene65, computed once"""
    md, pm, x0, _ = cases.scene65()
    ref64, s64 = oracle_optimize(x0, pm, iter_num=3)
    ref32, s32 = oracle_optimize(x0, pm, torch.float32, iter_num=3)
    assert s64 == s32 == 6
    gd64, steps64 = oracle_guide(x0, md, GUIDE_CFG)
    gd32, _ = oracle_guide(x0, md, GUIDE_CFG, torch.float32)
    return ref64, ref32, gd64, gd32, steps64


@pytest.fixture(scope="module")
def host65(eng):
    """results of the host-uploaded 65-frame scene at the default workgroup count (shared by tests 1, 2, 4 and 6; never modified)"""
    md, _, x0, _ = cases.scene65()
    _upload(eng, 0, md)
    return _run(eng, x0.to(DEV))


# ------------------------------------------------------------------------------------------------ 1. against fp64
def test_pairs_of_several_items_at_65_frames_vs_fp64(eng, host65):
    """Raises on the parent commit: the option does not exist there, and the plan refuses a pair of more than 512 matches."""
    md, pm, x0, _ = cases.scene65()
    _upload(eng, 0, md)
    p = eng.ggs_plan(1, 65, make_ggs_cfg())
    assert p[3] == 3 and p[0] == 256, p                                   # pd_ggs_longm_kernel, 256 workgroups
    loss, grad, out, st, g, stg = host65
    assert int(loss[0, 1]) == cases.SCENE65_FIGURES["valid"], loss
    eg, bg = check_loss_grad(loss[0].cpu(), grad.cpu(), x0, pm, "n65_pair_items")
    ref64, ref32, gd64, gd32, steps64 = _oracle65()
    assert int(st[0, 1]) == 6, st
    es, bs = check_steps(out, x0, ref64, ref32, "n65_pair_items")
    assert stg[0, :, 1].long().tolist() == steps64 == [4, 2, 2, 2, 4], (stg[0, :, 1].tolist(), steps64)
    eu, bu = check_steps(g, x0, gd64, gd32, "n65_pair_items/guide")
    fmt = lambda d: {k: f"{v:.1e}" for k, v in d.items()}
    print(f"\nplan {p}; valid {int(loss[0, 1])}; gradient {fmt(eg)} (bound {fmt(bg)}); step {fmt(es)} (bound {fmt(bs)}); "
          f"guide {fmt(eu)} (bound {fmt(bu)})")


# ------------------------------------------------------------------------------------------------ 2. workgroup count
@pytest.mark.parametrize("wgs", [3, 17])
def test_results_do_not_depend_on_the_workgroup_count(eng, host65, wgs):
    md, _, x0, _ = cases.scene65()
    _upload(eng, 0, md)
    p = eng.ggs_plan(1, 65, make_ggs_cfg(wgs_per_seq=wgs))
    assert p[3] == 3 and p[0] == wgs, p
    if wgs == 3:
        assert p[1] == 696, p              # 87 rounds of 8 slots, run in batches (tests/test_kernel_resources_ggs_long.py): the big pairs sit in
        #                                    rounds 0, 9, 27 and 86 of their workgroups, which a batch of <= 512 slots (64 rounds) cannot all hold
    res = _run(eng, x0.to(DEV), wgs_per_seq=wgs)
    _same_update(res, host65, ("wgs", wgs))
    print(f"\nwgs_per_seq = {wgs}: plan {p}; loss row bitwise: {torch.equal(res[0], host65[0])}")


# ------------------------------------------------------------------------------------------------ 3. a single-item pair is untouched
def test_single_item_tables_through_the_new_kernel_are_bitwise_the_long_kernel(eng):
    _, _, x0, base = cases.scene65()
    x = x0.to(DEV)
    _upload(eng, 0, base)
    p_old = eng.ggs_plan(1, 65, make_ggs_cfg())
    assert p_old[3] == 2 and p_old[0] == 256, p_old                       # pd_ggs_long_kernel
    old = _run(eng, x)
    _ingest(eng, 0, base, max_matches_per_pair=0)                         # no hint: the host shadow is not one item per pair
    p_new = eng.ggs_plan(1, 65, make_ggs_cfg())
    assert p_new[3] == 3 and p_new[0] == 256, p_new
    new = _run(eng, x)
    for i, (a, b) in enumerate(zip(old, new)):
        assert torch.equal(a, b), i
    assert float(old[0][0, 1]) > 0 and torch.isfinite(old[1]).all()


# ------------------------------------------------------------------------------------------------ 4. mixed launch
def test_mixed_launch_gives_every_slot_what_it_gives_alone(eng, host65):
    md65, _, x65, _ = cases.scene65()
    md40, _, x40 = cases.scene40()
    _upload(eng, 0, md40)
    assert eng.ggs_plan(1, 40, make_ggs_cfg(reserved=LONG))[3] == 2       # alone: pd_ggs_long_kernel
    alone40 = _run(eng, x40.to(DEV), reserved=LONG)
    _upload(eng, 0, md65)
    _upload(eng, 1, md40)
    counts = [65, 40]
    p = eng.ggs_plan(2, 65, make_ggs_cfg(), n_frames=counts)
    assert p[3] == 3, p
    x = torch.zeros(2, 65, 9)
    x[0], x[1, :40] = x65[0], x40[0]
    res = _run(eng, x.to(DEV), n_frames=counts)
    _same_update(res, host65, "slot 0", rows=slice(0, 1), rows_b=slice(0, 1))
    _same_update(res, alone40, "slot 1", rows=slice(1, 2), rows_b=slice(0, 1), frames=40)
    assert torch.equal(res[2][1, 40:], x[1, 40:].to(DEV))                 # padding rows are not touched


# ------------------------------------------------------------------------------------------------ 5. 33 frames
def test_33_frames_under_the_long_frames_flag_vs_fp64(eng):
    """Scene seed 833 (tests/ggs_pair_items_cases.py), chosen from the oracle alone: the fp64 and fp32 oracles count the same 5 762 valid
    matches at the start point, the Sampson value nearest the threshold is 2.07e-4 relative away from it (outside the 1e-4 band of
    ggs_checks.sampson_max_for), and both step all 6 iterations.  528 pairs on 66 workgroups: 8 slots each, so single-item pairs keep
    their matches in registers while the pairs of 600 and 1 100 matches stream theirs."""
    md, pm, x0 = cases.scene33()
    _upload(eng, 0, md)
    p = eng.ggs_plan(1, 33, make_ggs_cfg(reserved=LONG))
    assert p[3] == 3 and p[1] == 8 and p[0] == 66, p
    x = x0.to(DEV)
    loss, grad = eng.ggs_loss_grad(x, cfg=make_ggs_cfg(reserved=LONG))
    out, st, _ = eng.ggs_optimize(x, cfg=make_ggs_cfg(iter_num=3, reserved=LONG))
    eng.check_async()
    assert int(loss[0, 1]) == cases.SCENE33_FIGURES["valid"], loss
    check_loss_grad(loss[0].cpu(), grad.cpu(), x0, pm, "n33_pair_items")
    ref64, s64 = oracle_optimize(x0, pm, iter_num=3)
    ref32, s32 = oracle_optimize(x0, pm, torch.float32, iter_num=3)
    assert int(st[0, 1]) == s64 == s32 == 6, (st, s64, s32)
    check_steps(out, x0, ref64, ref32, "n33_pair_items")


# ------------------------------------------------------------------------------------------------ 6. device-built tables
@pytest.mark.parametrize("hint", [0, 1500])
def test_device_built_tables_are_bitwise_the_host_built(eng, host65, hint):
    md, _, x0, _ = cases.scene65()
    _ingest(eng, 0, md, max_matches_per_pair=hint)
    p = eng.ggs_plan(1, 65, make_ggs_cfg())
    assert p[3] == 3 and p[0] == 256, p
    res = _run(eng, x0.to(DEV))
    for i, (a, b) in enumerate(zip(res, host65)):
        assert torch.equal(a, b), (hint, i)


def test_violated_hint_above_512_raises_the_async_error_word(eng, host65):
    md, _, x0, _ = cases.scene65()
    _ingest(eng, 0, md, max_matches_per_pair=1024)                        # the pairs of 1 025 and 1 500 matches exceed it
    with pytest.raises(RuntimeError, match="pd_match_hints violated"):
        eng.check_async()
    eng.check_async()                                                     # cleared
    _ingest(eng, 0, md, max_matches_per_pair=1500)
    res = _run(eng, x0.to(DEV))
    for i, (a, b) in enumerate(zip(res, host65)):
        assert torch.equal(a, b), i


# ------------------------------------------------------------------------------------------------ 7. guided sampling
def test_guided_sampling_graph_equals_eager_and_is_keyed_on_the_plan(eng):
    N = 65
    md, _, _, base = cases.scene65()
    _upload(eng, 0, md)
    z = synth.make_z(1, N, seed=51).to(DEV)
    noise = torch.randn(101, 1, N, 9, generator=torch.Generator().manual_seed(52)).to(DEV)
    pose_g, proc_g, st_g = eng.sample(z, noise, 2, GUIDE_CFG, use_graph=True)
    pose_e, proc_e, st_e = eng.sample(z, noise, 2, GUIDE_CFG, use_graph=False)
    eng.check_async()
    assert torch.isfinite(pose_g).all() and torch.isfinite(proc_g).all()
    assert torch.equal(pose_g, pose_e) and torch.equal(proc_g, proc_e) and torch.equal(_nan0(st_g), _nan0(st_e))
    assert not torch.equal(proc_g[-1], proc_g[-3])                        # the guided steps moved the poses
    # single-item tables into the same slot: another plan (pd_ggs_long_kernel), so the multi-item graph must not be replayed
    _upload(eng, 0, base)
    assert eng.ggs_plan(1, N, make_ggs_cfg(GUIDE_CFG))[3] == 2
    pose_g2, proc_g2, st_g2 = eng.sample(z, noise, 2, GUIDE_CFG, use_graph=True)
    pose_e2, proc_e2, st_e2 = eng.sample(z, noise, 2, GUIDE_CFG, use_graph=False)
    eng.check_async()
    assert torch.equal(pose_g2, pose_e2) and torch.equal(proc_g2, proc_e2) and torch.equal(_nan0(st_g2), _nan0(st_e2))


# ------------------------------------------------------------------------------------------------ 8. option and refusals
def test_option_values_and_refusals_with_the_option_off(seeded_diffuser):
    e = _engine(seeded_diffuser.to(torch.device(DEV)), 1, 65, ggs_max_frames=65)
    try:
        assert e.get_option(OPT) == 0 and e.ggs_long_pair_items is False
        enc = synth.make_cameras(20, seed=5)
        md20 = synth.make_matches(enc, 224, 224, per_pair=40, seed=5)
        x20 = torch.as_tensor(enc).reshape(1, 20, 9).float().to(DEV)
        cfg20 = make_ggs_cfg(GUIDE_CFG)

        def at_20():
            _upload(e, 0, md20)
            g, st = e.ggs_guide(x20, 3, cfg20)
            e.check_async()
            return g, st

        g_ref, st_ref = at_20()

        def works_at_20():
            g, st = at_20()
            assert torch.equal(g, g_ref) and torch.equal(st, st_ref)

        for bad in (2, -1):
            with pytest.raises(RuntimeError, match=rf"code -1.*PD_OPT_GGS_LONG_PAIR_ITEMS.*got {bad}"):
                e.set_option(OPT, bad)
            assert e.get_option(OPT) == 0
            works_at_20()
        md, _, x0, _ = cases.scene65()
        _upload(e, 0, md)
        with pytest.raises(RuntimeError, match=r"code -2.*slot 0.*more than 512 matches"):       # today's message
            e.ggs_loss_grad(x0.to(DEV), cfg=make_ggs_cfg())
        works_at_20()
        with pytest.raises(RuntimeError, match=r"code -2.*max_matches_per_pair"):
            _ingest(e, 0, md, max_matches_per_pair=0)
        works_at_20()
        # switched on, the tables uploaded before stay valid; switched off again, the refusal is back
        _upload(e, 0, md)
        e.set_option(OPT, 1)
        assert e.get_option(OPT) == 1 and e.ggs_plan(1, 65, make_ggs_cfg())[3] == 3
        loss, _ = e.ggs_loss_grad(x0.to(DEV), cfg=make_ggs_cfg())
        e.check_async()
        assert int(loss[0, 1]) == cases.SCENE65_FIGURES["valid"]
        e.set_option(OPT, 0)
        with pytest.raises(RuntimeError, match=r"code -2.*slot 0.*more than 512 matches"):
            e.ggs_plan(1, 65, make_ggs_cfg())
        works_at_20()
    finally:
        e.close()
