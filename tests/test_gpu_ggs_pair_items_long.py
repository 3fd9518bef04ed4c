"""GPU (-m gpu): pd_ggs_longm_kernel (PD_OPT_GGS_LONG_PAIR_ITEMS: frame pairs of more than 512 matches above 64 frames) and the tables both
builders write for it, from 66 to 256 frames -- what tests/test_gpu_ggs_pair_items.py pins at 65 frames only.  Two engines of max_B = 3,
max_N = 256, ggs_max_frames = 256 with the option on sit side by side: one takes every sequence through the host builder
(pd_ggs_set_matches), the other through the device (pd_ggs_set_matches_csr_async_nf).  The scenes are cases.long_scene(..) of
tests/ggs_pair_items_cases.py: their rows are shuffled, so every big pair's rows are scattered over the whole upload; their oracle-side
figures, and that the checks used here can see every single work item, are pinned on the CPU by tests/test_ggs_pair_items_cpu.py.
Tolerances are those of tests/ggs_checks.py.

  a. against fp64, host upload, 256 workgroups: scene129 (40 slots per workgroup: 5 rounds, a big pair in each, the last pair of the
     table one of 5 items), scene256 (128 slots: 16 rounds), scene100_both (both orders of a pair multi-item with different counts)
  b. scene129 on 17 and 64 workgroups is bitwise the default; on 17 a workgroup's 488 slots run in several batches
  c. device-built tables are bitwise the host-built ones: hints 0 / exact / exact with max_pairs and one_order, pinned and device inputs;
     a hint one below the largest pair raises the asynchronous error word
  d. ragged: (100, 70, 40) frames, all multi-item, in one ingest call and one launch; every slot bitwise what it gives alone
  e. re-upload of 256, then 40, then 129 frames into one slot without waiting

"Bitwise" where the workgroup count differs (b, d) is what test_gpu_ggs_pair_items.py's docstring says (`_same_update`): gradient, valid
count, poses, iterations; the printed loss means are sums of per-workgroup totals and are held to the 1e-6 relative of `_loss_close`.
The guide oracle is computed for scene129 and scene100_both only (its CPU time: tests/test_ggs_pair_items_cpu.py).
"""
import functools
import time

import pytest
import torch

import ggs_pair_items_cases as cases
from ggs_checks import check_loss_grad, check_steps, oracle_guide, oracle_optimize
from posediffusion_amd import _lib
from posediffusion_amd.engine import PoseEngine, make_ggs_cfg
from posediffusion_amd.host import denoiser_state, pack_matches_ragged
from test_gpu_ggs_pair_items import _run, _same_update

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LONG = _lib.PD_GGS_CFG_LONG_FRAMES
GUIDE_CFG = cases.GUIDE_CFG
LDS_CU = 160 * 1024


def _engine(diff):
    e = PoseEngine(denoiser_state(diff.model), {k: v for k, v in diff.named_buffers(recurse=False)}, device=torch.device(DEV),
                   max_B=3, max_N=256, ggs_max_frames=256, ggs_long_pair_items=True)
    assert e.ggs_max_frames == 256 and e.ggs_long_pair_items is True
    return e


@pytest.fixture(scope="module")
def engines(seeded_diffuser):
    t0 = time.time()
    diff = seeded_diffuser.to(torch.device(DEV))
    e_host, e_dev = _engine(diff), _engine(diff)
    yield e_host, e_dev
    e_host.close()
    e_dev.close()
    print(f"\ntests/test_gpu_ggs_pair_items_long.py: {time.time() - t0:.1f} s from the engines' construction to their close")


def _host(eng, mds, slot=0):
    for b, md in enumerate(mds):
        eng.set_matches(slot + b, md["kp1"], md["kp2"], md["i12"], md["img_shape"])


def _ingest(eng, mds, where="pinned", slot=0, **hints):
    """ONE device-side call for the sequences `mds` into slots slot .."""
    kp1, kp2, i12, off, shape, counts = pack_matches_ragged(mds, pin=True)
    if where == "device":
        kp1, kp2, i12 = (t.to(DEV, non_blocking=True) for t in (kp1, kp2, i12))
    eng.set_matches_async(slot, kp1, kp2, i12, off, shape, n_frames=counts, **hints)


def _max_per_pair(name):
    return max(cases.LONG_SCENES[name][3].values())


def _padded(x0s):
    x = torch.zeros(len(x0s), max(x.shape[1] for x in x0s), 9)
    for b, x0 in enumerate(x0s):
        x[b, :x0.shape[1]] = x0[0]
    return x.to(DEV)


def _all_equal(a, b, tag):
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), (tag, i)


def _fmt(d):
    return {k: f"{v:.1e}" for k, v in d.items()}


@pytest.fixture(scope="module")
def host_alone(engines):
    """results of a scene host-uploaded into slot 0 and run alone at the default workgroup count, computed once each and never modified:
    host_alone(name, reserved=0) -> (plan, _run's outputs).  The call leaves the scene in slot 0 of the host engine."""
    e_host, _ = engines
    cache = {}

    def get(name, reserved=0):
        md, _, x0 = cases.long_scene(name)
        _host(e_host, [md])
        if (name, reserved) not in cache:
            N = x0.shape[1]
            cache[name, reserved] = (e_host.ggs_plan(1, N, make_ggs_cfg(reserved=reserved)), _run(e_host, x0.to(DEV), reserved=reserved))
        return cache[name, reserved]

    return get


@functools.lru_cache(maxsize=None)
def _oracle(name, guide):
    """the fp64 / fp32 oracle's 3 iterations (and shortened guide) of a scene, computed once"""
    md, pm, x0 = cases.long_scene(name)
    ref64, s64 = oracle_optimize(x0, pm, iter_num=3)
    ref32, s32 = oracle_optimize(x0, pm, torch.float32, iter_num=3)
    assert s64 == s32 == 6
    if not guide:
        return ref64, ref32, None, None, None
    gd64, steps64 = oracle_guide(x0, md, GUIDE_CFG)
    gd32, _ = oracle_guide(x0, md, GUIDE_CFG, torch.float32)
    return ref64, ref32, gd64, gd32, steps64


def _vs_fp64(name, res, guide, tag):
    """loss + gradient, 3 iterations and (guide) the shortened guide of ONE sequence against the fp64 oracle; prints errors and bounds"""
    _, pm, x0 = cases.long_scene(name)
    F = cases.LONG_FIGURES[name]
    loss, grad, out, st, g, stg = res
    assert int(loss[0, 1]) == F["valid"], (tag, loss)
    eg, bg = check_loss_grad(loss[0].cpu(), grad.cpu(), x0, pm, tag)
    ref64, ref32, gd64, gd32, steps64 = _oracle(name, guide)
    assert int(st[0, 1]) == 6, (tag, st)
    es, bs = check_steps(out, x0, ref64, ref32, tag)
    line = f"valid {int(loss[0, 1])}; gradient {_fmt(eg)} (bound {_fmt(bg)}); step {_fmt(es)} (bound {_fmt(bs)})"
    worst = max(max(eg[k] / bg[k] for k in eg), max(es[k] / bs[k] for k in es))
    if guide:
        assert stg[0, :, 1].long().tolist() == steps64 == F["guide_steps"], (tag, stg[0, :, 1].tolist(), steps64)
        eu, bu = check_steps(g, x0, gd64, gd32, tag + "/guide")
        line += f"; guide {_fmt(eu)} (bound {_fmt(bu)})"
        worst = max(worst, max(eu[k] / bu[k] for k in eu))
    print(f"\n{tag}: {line}; worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ a. against fp64
@pytest.mark.parametrize("name, slots, guide", [("scene129", 40, True), ("scene256", 128, False), ("scene100_both", 40, True)])
def test_pairs_of_several_items_above_65_frames_vs_fp64(host_alone, name, slots, guide):
    """scene129: p = wg*8 + (s&7) + (s>>3)*2048 with s >> 3 up to 4, a big pair in every round, two in workgroup 7, the pair of 1 536
    matches (3 full items: the clamp of the match index never acts) and the LAST pair of the table with 5 items.  scene256: s >> 3 up to
    15, pair ranks up to 32 639.  scene100_both: 9 900 ordered pairs on 256 workgroups are 5 rounds (40 slots); (7, 50) and (50, 7) hold 2
    and 3 items, every frame 198 incidence rows."""
    plan, res = host_alone(name)
    assert plan[3] == 3 and plan[0] == 256 and plan[1] == slots, plan               # pd_ggs_longm_kernel, 256 workgroups x slots
    print(f"\n{name}: plan {plan}")
    _vs_fp64(name, res, guide, name)


# ------------------------------------------------------------------------------------------------ b. workgroup count
def _one_batch_image(plans, slots):
    """LDS bytes of the image that would hold `slots` slots in ONE batch, from two reported one-batch plans: carve_long is linear in the slot
    count there (csrc/pd_ggs_lds.h)"""
    (s0, b0), (s1, b1) = [(p[1], p[2]) for p in plans]
    per_slot = (b1 - b0) // (s1 - s0)
    assert (b1 - b0) % (s1 - s0) == 0 and per_slot > 0
    return b0 + (slots - s0) * per_slot


def test_results_do_not_depend_on_the_workgroup_count_at_129_frames(engines, host_alone):
    e_host, _ = engines
    _, _, x0 = cases.long_scene("scene129")
    p256, ref = host_alone("scene129")
    compared, plans = [], {256: p256}
    for first in (17, 64):
        wgs = first
        while True:                                    # a refused count (code -2): assert the refusal, take the next larger power of two
            try:
                p = e_host.ggs_plan(1, 129, make_ggs_cfg(wgs_per_seq=wgs))
                break
            except RuntimeError as err:
                assert "code -2" in str(err), err
                wgs = 1 << wgs.bit_length()
                assert wgs < 256 and wgs not in compared, (first, wgs)
        assert p[3] == 3 and p[0] == wgs and p[1] == -(-8256 // (8 * wgs)) * 8, p
        res = _run(e_host, x0.to(DEV), wgs_per_seq=wgs)
        _same_update(res, ref, ("wgs", wgs))
        compared.append(wgs)
        plans[wgs] = p
        print(f"\nscene129 wgs_per_seq = {wgs}: plan {p}; loss row bitwise: {torch.equal(res[0], ref[0])}")
    assert len(set(compared)) >= 2, compared
    # several batches: the plan's LDS image is smaller than the one-batch image of its slots, which a CU cannot hold (or a batch is capped
    # at one slot per thread, 512).  The one-batch image is extrapolated from the two largest workgroup counts' plans, both one batch.
    small = sorted(plans)[-2:]
    assert all(plans[w][1] <= 512 and plans[w][2] <= LDS_CU for w in small)
    batched = []
    for w in compared:
        whole = _one_batch_image([plans[v] for v in small], plans[w][1])
        assert plans[w][2] <= LDS_CU, plans[w]
        if whole > LDS_CU or plans[w][1] > 512:
            assert plans[w][2] < whole, (plans[w], whole)
            batched.append((w, plans[w][1], plans[w][2], whole))
    print(f"\nslots in several batches (wgs, slots, LDS bytes, one-batch image): {batched}")
    assert batched, plans


# ------------------------------------------------------------------------------------------------ c. device-built tables
def _hints(name, kind):
    N, _, ordered, _, _ = cases.LONG_SCENES[name]
    if kind == "none":
        return dict(max_matches_per_pair=0)
    h = dict(max_matches_per_pair=_max_per_pair(name))
    if kind == "exact_pairs_order":                      # (one_order only where it is true: the hint is checked on the device)
        h.update(max_pairs=cases.LONG_FIGURES[name]["pairs"], one_order=not ordered)
    return h


@pytest.mark.parametrize("kind, where", [("none", "pinned"), ("exact", "device"), ("exact_pairs_order", "pinned")])
@pytest.mark.parametrize("name", ["scene129", "scene256", "scene100_both"])
def test_device_built_tables_of_scattered_big_pairs_are_bitwise_the_host_built(engines, host_alone, name, kind, where):
    """The rows of a big pair come back together only through the sort (many tiles of 1 024 rows, two passes above 64 frames, keys i*N + j
    up to 65 535), and a pair's items are cut from its rows in upload order: a sort that is not stable changes the bits."""
    _, e_dev = engines
    md, _, x0 = cases.long_scene(name)
    plan, ref = host_alone(name)
    _ingest(e_dev, [md], where, **_hints(name, kind))
    p = e_dev.ggs_plan(1, x0.shape[1], make_ggs_cfg())
    # without max_pairs the device engine sizes the slot table for every ordered pair it may meet: more slots, the same workgroups
    assert p[3] == 3 and p[0] == plan[0] and (p[1] == plan[1] if kind == "exact_pairs_order" else p[1] >= plan[1]), (p, plan)
    _all_equal(_run(e_dev, x0.to(DEV)), ref, (name, kind, where))                 # (_run ends with check_async())


def test_hint_one_below_the_largest_pair_raises_the_async_error_word(engines, host_alone):
    _, e_dev = engines
    md, _, x0 = cases.long_scene("scene129")
    _, ref = host_alone("scene129")
    _ingest(e_dev, [md], "pinned", max_matches_per_pair=2048)                   # the last pair holds 2 049
    with pytest.raises(RuntimeError, match="pd_match_hints violated"):
        e_dev.check_async()
    e_dev.check_async()                                                         # cleared
    _ingest(e_dev, [md], "pinned", max_matches_per_pair=2049)
    _all_equal(_run(e_dev, x0.to(DEV)), ref, "correct upload after the violated hint")


# ------------------------------------------------------------------------------------------------ d. ragged
RAGGED = ("scene100_both", "scene70", "scene40_big")


def test_ragged_launch_of_three_multi_item_sequences(engines, host_alone):
    """Slots of 100, 70 and 40 frames, each with pairs of several items, through ONE ingest call and ONE padded launch.  The 40-frame slot
    alone would run the kernels for at most 64 frames; its longer neighbours pull it onto pd_ggs_longm_kernel."""
    e_host, e_dev = engines
    scenes = [cases.long_scene(n) for n in RAGGED]
    counts = [s[2].shape[1] for s in scenes]
    assert counts == [100, 70, 40]
    # every slot alone on this kernel (the 40-frame one under PD_GGS_CFG_LONG_FRAMES), and the 40-frame one alone on its own family
    alone = []
    for n in RAGGED:
        plan, res = host_alone(n, LONG if n == "scene40_big" else 0)
        assert plan[3] == 3, (n, plan)
        alone.append(res)
    md40, pm40, x40 = scenes[2]
    _host(e_host, [md40])
    p40 = e_host.ggs_plan(1, 40, make_ggs_cfg())
    assert p40[3] < 2, p40                                                      # not a kernel for more than 64 frames
    loss, grad = e_host.ggs_loss_grad(x40.to(DEV), cfg=make_ggs_cfg())
    out, st, _ = e_host.ggs_optimize(x40.to(DEV), cfg=make_ggs_cfg(iter_num=3))
    e_host.check_async()
    assert int(loss[0, 1]) == cases.SCENE40_BIG_FIGURES["valid"], loss
    eg, bg = check_loss_grad(loss[0].cpu(), grad.cpu(), x40, pm40, "scene40_big alone, kernels for at most 64 frames")
    ref64, ref32 = _oracle("scene40_big", False)[:2]
    assert int(st[0, 1]) == 6, st
    es, bs = check_steps(out, x40, ref64, ref32, "scene40_big alone, kernels for at most 64 frames")
    print(f"\nscene40_big alone: plan {p40}; gradient {_fmt(eg)} (bound {_fmt(bg)}); step {_fmt(es)} (bound {_fmt(bs)})")

    for order, hint in (((0, 1, 2), 0), ((2, 1, 0), max(_max_per_pair(n) for n in RAGGED))):
        mds = [scenes[b][0] for b in order]
        cnt = [counts[b] for b in order]
        x = _padded([scenes[b][2] for b in order])
        _host(e_host, mds)
        _ingest(e_dev, mds, "pinned" if hint else "device", max_matches_per_pair=hint)          # one call, n_frames = cnt
        p_h, p_d = (e.ggs_plan(3, 100, make_ggs_cfg(), n_frames=cnt) for e in (e_host, e_dev))
        assert p_h[3] == p_d[3] == 3 and p_h[0] == p_d[0] and p_d[1] >= p_h[1], (p_h, p_d)       # (no max_pairs hint: see test c)
        r_h, r_d = _run(e_host, x, n_frames=cnt), _run(e_dev, x, n_frames=cnt)
        _all_equal(r_h, r_d, ("ragged", cnt))
        print(f"\nragged {cnt}: plan {p_h}; valid {r_h[0][:, 1].long().tolist()}")
        for slot, b in enumerate(order):
            assert int(r_h[0][slot, 1]) == cases.LONG_FIGURES[RAGGED[b]]["valid"], (cnt, slot, r_h[0])
            _same_update(r_h, alone[b], ("slot", slot), rows=slice(slot, slot + 1), rows_b=slice(0, 1), frames=counts[b])
            for i in (2, 4):
                assert torch.equal(r_h[i][slot, counts[b]:], x[slot, counts[b]:]), (cnt, slot, i)   # padding rows are not touched


# ------------------------------------------------------------------------------------------------ e. re-upload without waiting
def test_reupload_256_then_40_then_129_frames_into_the_same_slot(engines, host_alone):
    _, e_dev = engines
    seq = (("scene256", 0), ("scene40_big", LONG), ("scene129", 0))
    for name, reserved in seq:
        md, _, x0 = cases.long_scene(name)
        plan, ref = host_alone(name, reserved)
        assert plan[3] == 3, (name, plan)
        _ingest(e_dev, [md], "device", max_matches_per_pair=_max_per_pair(name))      # no wait in between: ordered on the device
        _all_equal(_run(e_dev, x0.to(DEV), reserved=reserved), ref, ("reupload", name))
    for name, _ in seq:                                                                # all three uploads queued before anything runs
        _ingest(e_dev, [cases.long_scene(name)[0]], "pinned", max_matches_per_pair=0)
    _all_equal(_run(e_dev, cases.long_scene("scene129")[2].to(DEV)), host_alone("scene129")[1], "three uploads back to back")
