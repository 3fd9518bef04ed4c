"""GPU (-m gpu): device-side match ingestion with one frame count per sequence (pd_ggs_set_matches_csr_async_nf, the ingest_nf_* kernels of
csrc/pd_ggs_ingest.hip; ``PoseEngine.set_matches_async(..., n_frames=)``) -- sequences of 65 .. 256 frames and ragged batches in one call.

Two engines of max_B = 4, max_N = 256, ggs_max_frames = 256 sit side by side: one takes every sequence through the host builder
(pd_ggs_set_matches), the other through the device.  "Bitwise" below: ``torch.equal`` on loss and gradient of ``ggs_loss_grad`` and on the
poses and statistics (after nan_to_num) of ``ggs_optimize(iter_num=3)``, with ``check_async()`` clean, for ``wgs_per_seq`` in (0, 3, 17)
above 64 frames and (0, 1, 3) at or below.  Where pd_ggs_plan refuses a workgroup count for the HOST-uploaded sequence (3 workgroups cannot
hold the 9 900 pairs of 100 frames in LDS; see tests/test_kernel_resources_ggs_long.py) there is nothing to compare: the device-built slot
must then be refused as well.

  1. uniform counts above 64, rows shuffled (the sort's stability), device-resident and pinned inputs, two sets of hints
  2. counts (100, 40, 8) in one call; the 8-frame slot alone on the lane / one-hop kernels
  3. counts (20, 13, 8, 20) in one call: lane tables and results
  4. uniform counts <= 64 through the new export against the old export
  5. re-upload without waiting: 256, then 8, then 100 frames into the same slot
  6. errors that surface in the asynchronous error word      7. synchronous refusals      8. guided sampling at 65 frames
"""
import functools

import numpy as np
import pytest
import torch

from posediffusion_amd import _lib, synth
from posediffusion_amd.engine import PoseEngine, make_ggs_cfg
from posediffusion_amd.host import denoiser_state, pack_matches, pack_matches_ragged

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LONG_WGS, SHORT_WGS = (0, 3, 17), (0, 1, 3)


def _engine(diff, max_B=4, max_N=256, **kw):
    return PoseEngine(denoiser_state(diff.model), {k: v for k, v in diff.named_buffers(recurse=False)}, device=torch.device(DEV),
                      max_B=max_B, max_N=max_N, **kw)


@pytest.fixture(scope="module")
def engines(seeded_diffuser):
    diff = seeded_diffuser.to(torch.device(DEV))
    e_host, e_dev = _engine(diff, ggs_max_frames=256), _engine(diff, ggs_max_frames=256)
    yield e_host, e_dev
    e_host.close()
    e_dev.close()


def _shuffled(md, seed):
    perm = np.random.default_rng(seed).permutation(len(md["kp1"]))
    return {"kp1": md["kp1"][perm], "kp2": md["kp2"][perm], "i12": md["i12"][perm], "img_shape": md["img_shape"]}


@functools.lru_cache(maxsize=None)
def _scene(N, per_pair, ordered=False, shuffle=True):
    """(matches, start pose [1, N, 9]) of one synthetic sequence, rows shuffled"""
    enc = synth.make_cameras(N, seed=1000 + N)
    md = synth.make_matches(enc, 224, 224, per_pair=per_pair, seed=1000 + N, ordered_pairs=ordered)
    return (_shuffled(md, N) if shuffle else md), synth.perturb_pose(enc, seed=1010 + N)


@functools.lru_cache(maxsize=None)
def _scene_256():
    """256 frames x 3: every pair i < j, plus the reversed-order rows of frames i = 255 and i = 128 -- the highest keys, a frame (128) with rows in
    all three runs of its incidences, 65 536 keys"""
    N = 256
    enc = synth.make_cameras(N, seed=1256)
    md = synth.make_matches(enc, 224, 224, per_pair=3, seed=1256, ordered_pairs=True)
    i, j = md["i12"][:, 0], md["i12"][:, 1]
    keep = (i < j) | (i == 255) | (i == 128)
    md = {"kp1": md["kp1"][keep], "kp2": md["kp2"][keep], "i12": md["i12"][keep], "img_shape": md["img_shape"]}
    assert md["i12"][:, 0].max() == 255 and (md["i12"][:, 0] * N + md["i12"][:, 1]).max() == 255 * 256 + 254
    return _shuffled(md, N), synth.perturb_pose(enc, seed=1266)


@functools.lru_cache(maxsize=None)
def _scene_65_big(n_big):
    """the 65-frame scene with pair (3, 7) raised to n_big matches"""
    md, x0 = _scene(65, 8, shuffle=False)
    enc = synth.make_cameras(65, seed=1065)
    extra = synth.make_matches(enc[[3, 7]], 224, 224, per_pair=n_big - 8, seed=77)
    n = len(extra["kp1"])
    big = {"kp1": np.concatenate([md["kp1"], extra["kp1"]]), "kp2": np.concatenate([md["kp2"], extra["kp2"]]),
           "i12": np.concatenate([md["i12"], np.tile(np.array([[3, 7]], dtype=np.int64), (n, 1))]), "img_shape": md["img_shape"]}
    key = big["i12"][:, 0] * 65 + big["i12"][:, 1]
    assert np.bincount(key).max() == n_big
    return _shuffled(big, 65), x0


def _n_pairs(md):
    n = int(md["img_shape"][0])
    return len(np.unique(md["i12"][:, 0] * n + md["i12"][:, 1]))


def _per_pair(md):
    n = int(md["img_shape"][0])
    return int(np.bincount(md["i12"][:, 0] * n + md["i12"][:, 1]).max())


def _ingest(eng, mds, where="pinned", slot=0, ragged=True, **hints):
    """one device-side call for the sequences `mds` into slots slot ..; ragged: through n_frames= (the new export)"""
    if ragged:
        kp1, kp2, i12, off, shape, counts = pack_matches_ragged(mds, pin=True)
    else:
        (kp1, kp2, i12, off, shape), counts = pack_matches(mds, pin=True), None
    if where == "device":
        kp1, kp2, i12 = (t.to(DEV, non_blocking=True) for t in (kp1, kp2, i12))
    eng.set_matches_async(slot, kp1, kp2, i12, off, shape, n_frames=counts, **hints) if ragged else \
        eng.set_matches_async(slot, kp1, kp2, i12, off, shape, **hints)


def _host(eng, mds, slot=0):
    for b, md in enumerate(mds):
        eng.set_matches(slot + b, md["kp1"], md["kp2"], md["i12"], md["img_shape"])


def _padded(x0s):
    NP = max(x.shape[1] for x in x0s)
    x = torch.zeros(len(x0s), NP, 9)
    for b, x0 in enumerate(x0s):
        x[b, :x0.shape[1]] = x0[0]
    return x.to(DEV)


def _run(eng, x, wgs, n_frames, reserved=0):
    cfg = dict(wgs_per_seq=wgs, reserved=reserved)
    loss, grad = eng.ggs_loss_grad(x, cfg=make_ggs_cfg(**cfg), n_frames=n_frames)
    out, st, _ = eng.ggs_optimize(x, cfg=make_ggs_cfg(iter_num=3, **cfg), n_frames=n_frames)
    eng.check_async()
    return loss, grad, out, st.nan_to_num(-1.0)


def _bitwise(e_a, e_b, x, wgs_list, n_frames=None, tag="", rows=None, reserved=0):
    """GGS on both engines, slots 0 .. B-1; `rows`: sequences to compare (default: all).  Returns the workgroup counts that were compared."""
    B, N = x.shape[0], x.shape[1]
    compared = []
    for wgs in wgs_list:
        try:
            e_a.ggs_plan(B, N, make_ggs_cfg(wgs_per_seq=wgs, reserved=reserved), n_frames=n_frames)
        except RuntimeError as err:                         # the plan refuses this workgroup count for the host-built tables
            assert "code -2" in str(err), err
            with pytest.raises(RuntimeError, match="code -2"):
                e_b.ggs_plan(B, N, make_ggs_cfg(wgs_per_seq=wgs, reserved=reserved), n_frames=n_frames)
            continue
        ra, rb = _run(e_a, x, wgs, n_frames, reserved), _run(e_b, x, wgs, n_frames, reserved)
        for name, a, b in zip(("loss", "grad", "poses", "stats"), ra, rb):
            sel = slice(None) if rows is None else rows
            assert torch.equal(a[sel], b[sel]), (tag, wgs, name)
        assert torch.isfinite(ra[1]).all() and float(ra[0][:, 1].min()) > 0, (tag, wgs)       # a real result: valid matches everywhere
        compared.append(wgs)
    assert 0 in compared, (tag, compared)
    return compared


# ------------------------------------------------------------------------------------------------ 1. uniform counts above 64
UNIFORM = {
    #                     scene,                               one-order, inputs
    "n65_x8": (lambda: _scene(65, 8), True, "device"),                       # 2 080 pairs, 17 tiles of 1 024
    "n100_x3_both_orders": (lambda: _scene(100, 3, True), False, "pinned"),   # 9 900 pairs, 198 rows per frame
    "n129_x2_both_orders": (lambda: _scene(129, 2, True), False, "device"),
    "n256_x3": (_scene_256, False, "pinned"),
    "n65_pair_of_512": (lambda: _scene_65_big(512), True, "pinned"),
}


@pytest.mark.parametrize("hints", ["pairs_and_order", "per_pair_only"])
@pytest.mark.parametrize("case", list(UNIFORM))
def test_uniform_counts_above_64_are_bitwise_the_host_upload(engines, case, hints):
    e_host, e_dev = engines
    scene, one_order, where = UNIFORM[case]
    md, x0 = scene()
    N = int(md["img_shape"][0])
    if case == "n65_x8":
        assert _n_pairs(md) == 2080 and (len(md["kp1"]) + 1023) // 1024 == 17
    if case == "n100_x3_both_orders":
        assert _n_pairs(md) == 9900
    h = dict(max_matches_per_pair=_per_pair(md))
    if hints == "pairs_and_order":                          # (one_order only where it is true: the hint is checked on the device)
        h.update(max_pairs=_n_pairs(md), one_order=one_order)
    _host(e_host, [md])
    _ingest(e_dev, [md], where, **h)
    compared = _bitwise(e_host, e_dev, x0.to(DEV), LONG_WGS, tag=(case, hints))
    if N == 65:
        assert compared == [0, 3, 17], compared
    print(f"\n{case} / {hints}: {len(md['kp1'])} matches, {_n_pairs(md)} pairs, compared at wgs_per_seq {compared}")


# ------------------------------------------------------------------------------------------------ 2. counts (100, 40, 8) in one call
MIXED = ((100, 3), (40, 8), (8, 60))


def test_mixed_counts_100_40_8_in_one_call(engines):
    e_host, e_dev = engines
    scenes = [_scene(n, pp) for n, pp in MIXED]
    mds, counts = [s[0] for s in scenes], [n for n, _ in MIXED]
    x = _padded([s[1] for s in scenes])
    _host(e_host, mds)
    hints = dict(max_pairs=4950, one_order=True, max_matches_per_pair=60)       # one set for the call: the pair bound of its longest sequence
    _ingest(e_dev, mds, "device", **hints)
    # the ragged launch: one padded batch, every slot with its own count
    _bitwise(e_host, e_dev, x, LONG_WGS, n_frames=counts, tag="ragged")
    g_h, s_h = e_host.ggs_guide(x, 3, make_ggs_cfg(dict(synth.GGS_CFG, iter_num=2)), n_frames=counts)
    g_d, s_d = e_dev.ggs_guide(x, 3, make_ggs_cfg(dict(synth.GGS_CFG, iter_num=2)), n_frames=counts)
    e_dev.check_async()
    assert torch.equal(g_h, g_d) and torch.equal(s_h.nan_to_num(-1.0), s_d.nan_to_num(-1.0))
    # every slot alone (slot 0 is the one a B = 1 launch reads): the 100-frame one on the long kernel ...
    _bitwise(e_host, e_dev, x[:1], LONG_WGS, tag="slot0")
    # ... and the same three sequences in the order (8, 40, 100): the 8-frame slot, which shared its call with longer ones, on the one-hop
    # kernels and on the lane kernel, the 40-frame one on the two-hop kernel
    order = [2, 1, 0]
    _host(e_host, [mds[b] for b in order])
    _ingest(e_dev, [mds[b] for b in order], "pinned", **hints)
    assert e_dev.lane_tables(0) == e_host.lane_tables(0) and e_host.lane_tables(0)[0] > 0
    _bitwise(e_host, e_dev, x[2:3, :8].contiguous(), SHORT_WGS, tag="slot 8 frames")
    _bitwise(e_host, e_dev, x[2:3, :8].contiguous(), (0,), tag="slot 8 frames / lane kernel", reserved=_lib.PD_GGS_CFG_LANE_ITEMS)
    _host(e_host, [mds[1]])
    _ingest(e_dev, [mds[1], mds[0]], "pinned", **hints)
    _bitwise(e_host, e_dev, x[1:2, :40].contiguous(), SHORT_WGS, tag="slot 40 frames")


# ------------------------------------------------------------------------------------------------ 3. counts (20, 13, 8, 20) in one call
def test_mixed_short_counts_in_one_call(engines):
    e_host, e_dev = engines
    spec = ((20, 30), (13, 47), (8, 64), (20, 81))
    scenes = [_scene(n, pp) for n, pp in spec[:3]]
    enc = synth.make_cameras(20, seed=1520)
    scenes.append((_shuffled(synth.make_matches(enc, 224, 224, per_pair=81, seed=1520), 20), synth.perturb_pose(enc, seed=1530)))
    mds, counts = [s[0] for s in scenes], [n for n, _ in spec]
    _host(e_host, mds)
    _ingest(e_dev, mds, "pinned")
    for b in range(4):
        assert e_dev.lane_tables(b) == e_host.lane_tables(b), b
        assert e_host.lane_tables(b)[0] > 0, b
    _bitwise(e_host, e_dev, _padded([s[1] for s in scenes]), SHORT_WGS, n_frames=counts, tag="20/13/8/20")


# ------------------------------------------------------------------------------------------------ 4. uniform counts <= 64: the old export
@pytest.mark.parametrize("case", ["n20_x300", "n40_two_hop"])
def test_uniform_short_counts_are_bitwise_the_old_export(engines, seeded_diffuser, case):
    e_host, e_dev = engines
    if case == "n20_x300":
        N, pps, hints = 20, (300, 300), dict(max_pairs=190, max_matches_per_pair=512, one_order=True)
    else:
        N, pps, hints = 40, (6, 7), dict(max_pairs=780, max_matches_per_pair=64)
    scenes = []
    for b, pp in enumerate(pps):
        enc = synth.make_cameras(N, seed=1600 + N + b)
        md = synth.make_matches(enc, 224, 224, per_pair=pp, seed=1600 + N + b)
        scenes.append((_shuffled(md, b) if N == 40 else md, synth.perturb_pose(enc, seed=1610 + N + b)))
    mds = [s[0] for s in scenes]
    x = _padded([s[1] for s in scenes])
    e_old = _engine(seeded_diffuser.to(torch.device(DEV)), ggs_max_frames=256)
    try:
        _ingest(e_old, mds, "pinned", ragged=False, **hints)
        _ingest(e_dev, mds, "pinned", **hints)
        _host(e_host, mds)
        for b in range(2):
            assert e_dev.lane_tables(b) == e_old.lane_tables(b) == e_host.lane_tables(b)
        for wgs in SHORT_WGS:                                     # the same plan on both device-built engines (capacities from the same hints)
            cfg = make_ggs_cfg(wgs_per_seq=wgs)
            assert e_dev.ggs_plan(2, N, cfg) == e_old.ggs_plan(2, N, cfg), (case, wgs)
        _bitwise(e_old, e_dev, x, SHORT_WGS, tag=case + " / old export")
        _bitwise(e_host, e_dev, x, SHORT_WGS, tag=case + " / host")
    finally:
        e_old.close()


# ------------------------------------------------------------------------------------------------ 5. re-upload without waiting
def test_reupload_256_then_8_then_100_frames_into_the_same_slot(engines):
    e_host, e_dev = engines
    for scene, wgs in ((_scene_256(), (0,)), (_scene(8, 60), SHORT_WGS), (_scene(100, 3), (0, 17))):
        md, x0 = scene
        _host(e_host, [md])
        _ingest(e_dev, [md], "device", max_matches_per_pair=_per_pair(md))      # no wait in between: ordered on the device
        _bitwise(e_host, e_dev, x0.to(DEV), wgs, tag=("reupload", int(md["img_shape"][0])))


# ------------------------------------------------------------------------------------------------ 6. asynchronous errors
def test_bad_index_and_violated_hint_raise_the_async_error_word(engines):
    e_host, e_dev = engines
    scenes = [_scene(n, pp) for n, pp in MIXED]
    mds, counts = [s[0] for s in scenes], [n for n, _ in MIXED]
    x = _padded([s[1] for s in scenes])
    _host(e_host, mds)
    bad = [dict(md) for md in mds]
    bad[1]["i12"] = bad[1]["i12"].copy()
    bad[1]["i12"][5, 1] = 40                                     # a frame of the call (100 frames), not of its sequence (40)
    _ingest(e_dev, bad, "pinned", max_matches_per_pair=60)
    with pytest.raises(RuntimeError, match="frame index outside"):
        e_dev.check_async()
    e_dev.check_async()                                          # cleared
    _bitwise(e_host, e_dev, x, (0, 17), n_frames=counts, tag="slots beside the bad one", rows=[0, 2])
    loss, _ = e_dev.ggs_loss_grad(x, cfg=make_ggs_cfg(), n_frames=counts)
    assert float(loss[1, 1]) == 0.0                              # the emptied slot: no valid match
    # a pair of 513 matches under the hint 512
    big, x65 = _scene_65_big(513)
    _ingest(e_dev, [big], "pinned", max_matches_per_pair=512)
    with pytest.raises(RuntimeError, match="pd_match_hints violated"):
        e_dev.check_async()
    e_dev.check_async()
    md, x0 = _scene(65, 8)
    _host(e_host, [md])
    _ingest(e_dev, [md], "pinned", max_matches_per_pair=8)
    _bitwise(e_host, e_dev, x0.to(DEV), (0,), tag="good upload after the errors")


# ------------------------------------------------------------------------------------------------ 7. synchronous refusals
def _works_at_20(e_host, e_dev):
    md, x0 = _scene(20, 30)
    _host(e_host, [md])
    _ingest(e_dev, [md], "pinned")
    _bitwise(e_host, e_dev, x0.to(DEV), (0,), tag="20 frames after a refusal")


def test_synchronous_refusals_leave_the_engine_usable(engines, seeded_diffuser):
    e_host, e_dev = engines
    md, _ = _scene(65, 8)
    packed = pack_matches([md], pin=True)
    kp1, kp2, i12, off, shape = packed
    big_shape = (300, *shape[1:])                              # (img_shape[0] only has to be >= every count)

    def call(eng, counts, **hints):
        eng.set_matches_async(0, kp1, kp2, i12, off, big_shape, n_frames=counts, **hints)

    for count in (0, 257):
        with pytest.raises(RuntimeError, match=r"code -1.*pd_ggs_set_matches_csr_async_nf"):
            call(e_dev, [count], max_matches_per_pair=8)
        _works_at_20(e_host, e_dev)
    for hint in (0, 513):
        with pytest.raises(RuntimeError, match=r"code -2.*max_matches_per_pair"):
            call(e_dev, [65], max_matches_per_pair=hint)
        _works_at_20(e_host, e_dev)
    with pytest.raises(RuntimeError, match=r"code -2.*limited to 64 frames \(n_frames=65\).*pd_ggs_set_matches"):
        e_dev.set_matches_async(0, kp1, kp2, i12, off, shape)   # n_frames=None: the old call and its message
    _works_at_20(e_host, e_dev)
    e80 = _engine(seeded_diffuser.to(torch.device(DEV)), max_B=1, max_N=100)
    try:
        e80.set_option(_lib.PD_OPT_GGS_MAX_FRAMES, 80)
        with pytest.raises(RuntimeError, match=r"code -2.*limited to 80 frames \(N=90\)"):
            e80.set_matches_async(0, kp1, kp2, i12, off, (100, *shape[1:]), n_frames=[90], max_matches_per_pair=8)
        _works_at_20(e_host, e80)
    finally:
        e80.close()


# ------------------------------------------------------------------------------------------------ 8. guided sampling at 65 frames
def test_guided_sampling_at_65_frames_from_device_built_tables(engines):
    e_host, e_dev = engines
    N = 65
    md, _ = _scene(N, 8)
    _host(e_host, [md])
    _ingest(e_dev, [md], "device", max_pairs=_n_pairs(md), max_matches_per_pair=8, one_order=True)
    z = synth.make_z(1, N, seed=41).to(DEV)
    noise = torch.randn(101, 1, N, 9, generator=torch.Generator().manual_seed(42)).to(DEV)
    cfg = dict(synth.GGS_CFG, iter_num=2)
    pose_g, proc_g, st_g = e_dev.sample(z, noise, 2, cfg, use_graph=True)
    pose_e, proc_e, st_e = e_dev.sample(z, noise, 2, cfg, use_graph=False)
    pose_h, proc_h, st_h = e_host.sample(z, noise, 2, cfg, use_graph=False)
    e_dev.check_async()
    e_host.check_async()
    assert torch.isfinite(pose_g).all() and not torch.equal(proc_g[-1], proc_g[-3])      # the guided steps moved the poses
    assert torch.equal(pose_g, pose_e) and torch.equal(proc_g, proc_e) and torch.equal(st_g.nan_to_num(-1.0), st_e.nan_to_num(-1.0))
    assert torch.equal(pose_e, pose_h) and torch.equal(proc_e, proc_h) and torch.equal(st_e.nan_to_num(-1.0), st_h.nan_to_num(-1.0))


# ------------------------------------------------------------------------------------------------ 9. host.upload_matches(device_side=True)
def test_upload_matches_device_side_is_one_ragged_call_and_caches(engines, monkeypatch):
    from posediffusion_amd.host import upload_matches
    e_host, e_dev = engines
    scenes = [_scene(n, pp) for n, pp in MIXED]
    mds, counts = [s[0] for s in scenes], [n for n, _ in MIXED]
    calls = []
    real = e_dev.set_matches_async
    monkeypatch.setattr(e_dev, "set_matches_async", lambda *a, **kw: (calls.append(kw.get("n_frames")), real(*a, **kw))[1])
    _host(e_dev, [_scene(20, 30)[0]])                             # (whatever the slots held: the identity cache is dropped by an upload)
    upload_matches(e_host, mds, 3, n_frames=counts)
    upload_matches(e_dev, mds, 3, n_frames=counts, device_side=True)
    upload_matches(e_dev, mds, 3, n_frames=counts, device_side=True)       # the same arrays: nothing to do
    assert calls == [counts], calls
    _bitwise(e_host, e_dev, _padded([s[1] for s in scenes]), (0, 17), n_frames=counts, tag="upload_matches(device_side=True)")
