"""GPU (-m gpu): GGS on non-square images and outside the clipped-step regime, per kernel family, against the fp64 oracle.

The scenes, the settings of (alpha, learning_rate, momentum), the iteration counts and the shared fp64 / fp32 references are those of
tests/ggs_input_cases.py (its docstring says how each was fixed on the CPU oracle); tests/test_ggs_inputs_cpu.py asserts without a GPU
that the regimes hold, that no match lies within the contract band of sampson_max wherever a valid count is compared here, and that the
checks used here fail on the errors they are for (h and w exchanged, a wrong learning_rate, a doubled in-loop gradient, a wrong momentum).
Every bound is one of tests/ggs_checks.py (K_* / FLOOR_*), TOL = 2e-5 or the fixture bounds of tests/test_gpu_parity.py.

  1. Image geometry: 192 x 320, 320 x 192, 96 x 512 and 1080 x 1920 at 6 frames (lane kernel, one workgroup of waves, one-hop with 3
     workgroups) and 33 frames (two-hop with the default and 17 workgroups, the long kernel through PD_GGS_CFG_LONG_FRAMES); both
     orientations at 65 frames (the long kernel on its own terms, ggs_max_frames raised).  The family pd_debug_ggs_plan reports is
     asserted.  Per (family, shape): loss, valid count and gradient; 3 iterations of GGS_optimize with all groups and with FL, R, T
     alone (FL alone is where cx / cy enter the gradient alone); one geometry_guided_sampling of [4, 2, 2, 2, 4] iterations.
  2. The engine against tests/golden/ggs_inputs.npz (the reference executed in place at 192 x 320 and three optimiser settings).
  3. Device-built match tables (pd_ggs_set_matches_csr_async) at 320 x 192, 6 and 33 frames: bit for bit the host upload's results.
  4. One launch of B = 3 whose slots were uploaded for 224 x 224, 192 x 320 and 320 x 192, uniform and ragged (6, 5, 4 frames): every
     slot bit for bit the sequence run alone -- a kernel reads sc / cx / cy from the sequence's own descriptor.
  5. Optimiser regimes on the square 8-frame fixture scene and on the 192 x 320 scene at 6, 33 and 65 frames (the long kernel on its own
     terms: its frame sums cross waves only above 64 frames), and the two-hop kernel's crossing run at 33 frames, 96 x 512: default, never
     clipped, crossing, learning_rate alone changed, momentum 0.5 and 0.0.  Per (family, setting): GGS_optimize with all groups and each single
     group; for the all-groups stage the per-iteration trace -- pose of every iteration per column group, valid count, loss, and the
     gradient norm BEFORE the clip (which the clipped step hides) -- and one geometry_guided_sampling through the drop-in function.
"""
import numpy as np
import pytest
import torch

import ggs_input_cases as Cs
from conftest import pose_err, rel_err
from ggs_checks import check_loss_grad, check_steps, check_trace, engine_trace_rows
from posediffusion_amd import _lib
from posediffusion_amd.engine import PoseEngine, make_ggs_cfg
from posediffusion_amd.host import denoiser_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5
LANE, NOLANE, LONG = _lib.PD_GGS_CFG_LANE_ITEMS, _lib.PD_GGS_CFG_NO_LANE_ITEMS, _lib.PD_GGS_CFG_LONG_FRAMES
SMALL = {"lane": dict(wgs_per_seq=1, reserved=LANE), "wave": dict(wgs_per_seq=1, reserved=NOLANE), "one_hop_k3": dict(wgs_per_seq=3, reserved=NOLANE)}
FAMILIES = {                     # frames -> {name: cfg fields}; the family the plan must report is the name up to "_k"
    6: SMALL, 8: SMALL,
    33: {"two_hop_k0": dict(wgs_per_seq=0), "two_hop_k17": dict(wgs_per_seq=17), "long": dict(reserved=LONG)},
    65: {"long": {}},
}
REGIME_FAMILIES = {6: dict(SMALL, long=dict(reserved=LONG)), 8: dict(SMALL, long=dict(reserved=LONG)), 33: FAMILIES[33], 65: FAMILIES[65]}
_TABLE = {}                      # row label -> text; printed when the module is done (pytest -s): profiles/ggs_input_domain.txt
_id = lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)
_fmt = lambda d: "/".join(f"{d[g]:.1e}" for g in ("T", "quaternion", "logFL"))


@pytest.fixture(scope="module")
def eng(seeded_diffuser):
    dev = torch.device(DEV)
    diff = seeded_diffuser.to(dev)
    e = PoseEngine(denoiser_state(diff.model), {k: v for k, v in diff.named_buffers(recurse=False)}, device=dev, max_B=4, max_N=65,
                   ggs_max_frames=65)
    yield e
    e.close()
    if _TABLE:
        lines = ["GGS input domain: worst errors against fp64 per kernel family (T/quaternion/logFL), with the bound in force",
                 "  geometry rows: gradient | step of 3 iterations (worst over the stages all, FL, R, T) | step of one guide",
                 "  regime rows:   step of GGS_optimize (worst over the stages) | step of each traced iteration | |g| before the clip", ""]
        lines += [f"{k:46s} {v}" for k, v in sorted(_TABLE.items())]
        print("\n" + "\n".join(lines))


def _upload(eng, slot, md):
    eng.set_matches(slot, md["kp1"], md["kp2"], md["i12"], md["img_shape"])


def _family(eng, B, N, cfg, n_frames=None):
    p = eng.ggs_plan(B, N, cfg, n_frames=n_frames)
    return "lane" if p[6] else "long" if p[3] == 2 else "two_hop" if p[3] == 1 else "one_hop" if p[0] > 1 else "wave"


def _assert_family(eng, N, name, fields):
    cfg = make_ggs_cfg(**fields)
    fam = _family(eng, 1, N, cfg)
    assert fam == name.split("_k")[0], (N, name, fam, eng.ggs_plan(1, N, cfg))
    if "_k" in name and fields.get("wgs_per_seq", 0) > 0:
        assert eng.ggs_plan(1, N, cfg)[0] == fields["wgs_per_seq"], (name, eng.ggs_plan(1, N, cfg))


def _worse(a, b):
    return b if a is None else {g: max(a[g], b[g]) for g in b}


# ------------------------------------------------------------------------------------------------ 1. image geometry
@pytest.mark.parametrize("key", Cs.GEOMETRY_SCENES, ids=_id)
def test_non_square_images_per_kernel_family_vs_fp64(eng, key):
    N, H, W = key
    md, pm, x0 = Cs.scene(*key)
    _upload(eng, 0, md)
    x = x0.to(DEV)
    cache = {}
    g64, g32, gsteps = Cs.guide_refs(key, "default")
    assert gsteps == [4, 2, 2, 2, 4]
    for name, fields in FAMILIES[N].items():
        tag = f"{_id(key)}/{name}"
        _assert_family(eng, N, name, fields)
        loss, grad = eng.ggs_loss_grad(x, cfg=make_ggs_cfg(**fields))
        eng.check_async()
        eg, bg = check_loss_grad(loss[0].cpu(), grad.cpu(), x0, pm, tag, cache)
        assert list(cache) == [int(loss[0, 1])], (tag, "valid count", list(cache), loss)        # one count: fp64's at sampson_max itself
        es = bs = None
        for fname, flags in Cs.FLAGS.items():
            r = Cs.optimize_refs(key, "default", fname)
            out, st, _ = eng.ggs_optimize(x, *flags, cfg=make_ggs_cfg(iter_num=Cs.ITER_NUM, **fields))
            eng.check_async()
            assert int(st[0, 1]) == r["steps64"] == r["steps32"] == (6 if fname == "all" else 3), (tag, fname, st)
            e, b = check_steps(out, x0, r["x64"], r["x32"], f"{tag}/{fname}")
            es, bs = _worse(es, e), _worse(bs, b)
        g, stg = eng.ggs_guide(x, 3, make_ggs_cfg(Cs.cfg_of("default", iter_num=Cs.GUIDE_ITER_NUM), **fields))
        eng.check_async()
        assert stg[0, :, 1].long().tolist() == gsteps, (tag, stg[0, :, 1].tolist())
        eu, bu = check_steps(g, x0, g64, g32, tag + "/guide")
        _TABLE[f"geometry {name:11s} {N:2d} x {H}x{W}"] = (f"grad {_fmt(eg)} (<= {_fmt(bg)}) | step {_fmt(es)} (<= {_fmt(bs)}) | "
                                                        f"guide {_fmt(eu)} (<= {_fmt(bu)})")


# ------------------------------------------------------------------------------------------------ 2. the reference's fixture
@pytest.mark.parametrize("setting", Cs.FIXTURE_SETTINGS)
def test_non_square_and_unclipped_vs_reference_fixture(eng, golden, setting):
    """Teacher-forced bounds of tests/test_gpu_parity.py (pose_err < 2e-5, gradient < 1e-4) on every family 6 frames reach."""
    g = golden["ggs_inputs"]
    key = Cs.FIXTURE_SCENE
    md, _, x0 = Cs.scene(*key)
    assert np.array_equal(g["kp1"], md["kp1"]) and np.array_equal(g["x0"], x0.numpy()) and tuple(g["img_shape"]) == tuple(md["img_shape"])
    cfg = Cs.cfg_of(setting, key)
    assert [cfg["alpha"], cfg["learning_rate"]] == g[f"{setting}_alpha_lr"].tolist()
    _upload(eng, 0, md)
    x = x0.to(DEV)
    for name, fields in REGIME_FAMILIES[6].items():
        _assert_family(eng, 6, name, fields)
        for fname, flags in Cs.FLAGS.items():
            if setting == "default":
                loss, grad = eng.ggs_loss_grad(x, *flags, cfg=make_ggs_cfg(**fields))
                assert int(loss[0, 1]) == int(g[f"sam_{fname}_nvalid"]), (name, fname)
                assert abs(float(loss[0, 0]) - float(g[f"sam_{fname}_loss"])) < TOL * float(g[f"sam_{fname}_loss"]), (name, fname)
                assert abs(float(loss[0, 2]) - float(g[f"sam_{fname}_print"])) < TOL * float(g[f"sam_{fname}_print"]), (name, fname)
                assert rel_err(grad, g[f"sam_{fname}_grad"]) < 1e-4, (name, fname)
            out, st, _ = eng.ggs_optimize(x, *flags, cfg=make_ggs_cfg(cfg, iter_num=3, **fields))
            eng.check_async()
            assert int(st[0, 1]) == (6 if fname == "all" else 3)
            assert pose_err(out, g[f"{setting}_opt_{fname}_k3"], f"ggs_inputs_{setting}_opt_{fname}") < TOL, (name, fname)
        out, st = eng.ggs_guide(x, 3, make_ggs_cfg(cfg, iter_num=2, **fields))
        eng.check_async()
        assert st[0, :, 1].long().tolist() == [4, 2, 2, 2, 4]
        assert pose_err(out, g[f"{setting}_guide_k2"], f"ggs_inputs_{setting}_guide") < TOL, name


# ------------------------------------------------------------------------------------------------ 3. device-built tables
@pytest.mark.parametrize("key", [(6, 320, 192), (33, 320, 192)], ids=_id)
def test_device_built_tables_on_a_non_square_image_are_the_host_built_ones(eng, key):
    N = key[0]
    md, _, x0 = Cs.scene(*key)
    x = x0.to(DEV)
    kp1, kp2, i12 = (torch.from_numpy(md[k]).to(DEV) for k in ("kp1", "kp2", "i12"))

    def run():
        res = []
        for name, fields in FAMILIES[N].items():
            _assert_family(eng, N, name, fields)
            loss, grad = eng.ggs_loss_grad(x, cfg=make_ggs_cfg(**fields))
            out, st, _ = eng.ggs_optimize(x, cfg=make_ggs_cfg(iter_num=3, **fields))
            fl, _, _ = eng.ggs_optimize(x, False, False, True, cfg=make_ggs_cfg(iter_num=3, **fields))
            g, stg = eng.ggs_guide(x, 3, make_ggs_cfg(Cs.cfg_of("default", iter_num=2), **fields))
            eng.check_async()
            res += [loss, grad, out, st.nan_to_num(-1.0), fl, g, stg.nan_to_num(-1.0)]
        return res

    _upload(eng, 0, md)
    host = run()
    eng.set_matches_async(0, kp1, kp2, i12, [0, kp1.shape[0]], md["img_shape"], max_pairs=N * (N - 1) // 2,
                          max_matches_per_pair=Cs.PER_PAIR[N], one_order=True)
    dev = run()
    assert int(host[0][0, 1]) > 0 and not torch.equal(host[2], x)
    for i, (a, b) in enumerate(zip(host, dev)):
        assert torch.equal(a, b), (key, i)


# ------------------------------------------------------------------------------------------------ 4. one mixed launch
SENTINEL = 7.25


@pytest.mark.parametrize("name", ["lane", "wave"])
def test_mixed_image_shapes_in_one_launch_equal_each_sequence_alone(eng, name):
    fields = SMALL[name]
    base, opt = make_ggs_cfg(**fields), make_ggs_cfg(iter_num=3, **fields)
    guide = make_ggs_cfg(Cs.cfg_of("default", iter_num=2), **fields)
    for keys, counts in ((Cs.MIXED_SCENES[:3], None), ([Cs.MIXED_SCENES[0]] + Cs.MIXED_SCENES[3:], (6, 5, 4))):
        scenes = [Cs.scene(*k) for k in keys]
        alone = []
        for k, (md, _, x0) in zip(keys, scenes):
            _upload(eng, 0, md)
            assert _family(eng, 1, k[0], base) == name, (k, name)
            xb = x0.to(DEV)
            loss, grad = eng.ggs_loss_grad(xb, cfg=base)
            out, st, _ = eng.ggs_optimize(xb, cfg=opt)
            fl, _, _ = eng.ggs_optimize(xb, False, False, True, cfg=opt)
            g, stg = eng.ggs_guide(xb, 3, guide)
            eng.check_async()
            assert int(st[0, 1]) == 6 and stg[0, :, 1].long().tolist() == [4, 2, 2, 2, 4], (k, st, stg)
            alone.append((loss[0], grad[0], out[0], st[0].nan_to_num(-1.0), fl[0], g[0], stg[0].nan_to_num(-1.0)))
        x = torch.full((3, 6, 9), SENTINEL)
        for b, (k, (md, _, x0)) in enumerate(zip(keys, scenes)):
            _upload(eng, b, md)
            x[b, :k[0]] = x0[0]
        x = x.to(DEV)
        assert _family(eng, 3, 6, base, counts) == name, (keys, name)
        loss, grad = eng.ggs_loss_grad(x, cfg=base, n_frames=counts)
        out, st, _ = eng.ggs_optimize(x, cfg=opt, n_frames=counts)
        fl, _, _ = eng.ggs_optimize(x, False, False, True, cfg=opt, n_frames=counts)
        g, stg = eng.ggs_guide(x, 3, guide, n_frames=counts)
        eng.check_async()
        for b, k in enumerate(keys):
            n = k[0]
            batch = (loss[b], grad[b, :n], out[b, :n], st[b].nan_to_num(-1.0), fl[b, :n], g[b, :n], stg[b].nan_to_num(-1.0))
            for i, (a, c) in enumerate(zip(alone[b], batch)):
                assert torch.equal(a, c), (name, keys, counts, b, i)
            assert bool((out[b, n:] == SENTINEL).all()) and bool((g[b, n:] == SENTINEL).all())
        assert not torch.equal(alone[0][0], alone[1][0])                     # (the slots hold different scenes)


# ------------------------------------------------------------------------------------------------ 5. optimiser regimes
@pytest.mark.parametrize("key,setting", [(k, s) for k in Cs.REGIME_SCENES for s in Cs.settings_of(k)], ids=_id)
def test_optimiser_regimes_per_kernel_family_vs_fp64(eng, monkeypatch, key, setting):
    N = key[0]
    md, _, x0 = Cs.scene(*key)
    _upload(eng, 0, md)
    x = x0.to(DEV)
    cfg = Cs.cfg_of(setting, key)
    iters = Cs.REGIME_ITER_NUM[N]
    for name, fields in REGIME_FAMILIES[N].items():
        tag = f"{_id(key)}/{setting}/{name}"
        _assert_family(eng, N, name, fields)
        es = bs = None
        for fname, flags in Cs.FLAGS.items():
            r = Cs.optimize_refs(key, setting, fname, iters)
            out, st, tr = eng.ggs_optimize(x, *flags, cfg=make_ggs_cfg(cfg, iter_num=iters, **fields), trace=(fname == "all"))
            eng.check_async()
            assert int(st[0, 1]) == r["steps64"] == iters * (2 if fname == "all" else 1), (tag, fname, st)
            e, b = check_steps(out, x0, r["x64"], r["x32"], f"{tag}/{fname}")
            es, bs = _worse(es, e), _worse(bs, b)
            if fname == "all":
                rows = engine_trace_rows(tr[0], N, 2 * iters)
                assert torch.equal(rows[-1][0], out[0].cpu().flatten()), tag                 # the last trace row is the result
                et, egn, bgn = check_trace(rows, x0, r["trace64"], r["trace32"], tag)
        _TABLE[f"regime {name:11s} {_id(key):10s} {setting}"] = (f"step {_fmt(es)} (<= {_fmt(bs)}) | per iteration {_fmt(et)} | "
                                                               f"gnorm {egn:.1e} (<= {bgn:.1e})")
    if "momentum" not in Cs.SETTINGS[setting]:
        # the drop-in function with the setting in its GGS_cfg dict and the scene's img_shape (the reference's cfg has no momentum field)
        from posediffusion_amd.dropin.util.geometry_guided_sampling import geometry_guided_sampling
        gcfg = dict(cfg, iter_num=Cs.GUIDE_ITER_NUM)
        g64, g32, gsteps = Cs.guide_refs(key, setting)
        monkeypatch.setenv("PD_GGS_VERBOSE", "0")
        g = geometry_guided_sampling(x, 3, md, gcfg, engine=eng)
        assert gsteps == [2 * Cs.GUIDE_ITER_NUM, Cs.GUIDE_ITER_NUM, Cs.GUIDE_ITER_NUM, Cs.GUIDE_ITER_NUM, 2 * Cs.GUIDE_ITER_NUM]
        eu, bu = check_steps(g, x0, g64, g32, f"{_id(key)}/{setting}/drop-in guide")
        _TABLE[f"regime {'drop-in':11s} {_id(key):10s} {setting}"] = f"guide {_fmt(eu)} (<= {_fmt(bu)})"
