"""GPU (-m gpu): the frame-count range the API admits (N <= PD_MAX_FRAMES = 64), on engines of max_N = 64.

  * GGS at N = 2, 24, 25, 32, 33, 64 and 64 with both orders of every pair (4 032 pairs: PD_GGS_MAX_PCHUNKS = 8 chunks): the thresholds
    PD_GGS_FAST_FRAMES = PD_LANE_MAX_FRAMES = 24, one -> two pair chunks at 33 frames (> 512 pairs) and the chunk ceiling.  Every kernel
    family the cfg can ask for (reserved = lane / no lane / forced one-hop / spread exchange x wgs_per_seq = 1, 0, 3, 17): the family
    pd_debug_ggs_plan reports is asserted, and value, valid count, gradient and the steps of 3 GGS_optimize iterations against the fp64
    oracle per column group (tests/ggs_checks.py); one shortened geometry_guided_sampling per case.
  * The denoiser above 32 frames and around the streamed path's 1 024 token rows, in both modes, against fp64.
  * A guided sampling pass at B = 2, N = 64: hipGraph replay equals eager launches.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_err
from ggs_checks import check_loss_grad, check_steps, oracle_guide, oracle_optimize
from oracle import pd_oracle as O
from posediffusion_amd import _lib, synth
from posediffusion_amd.engine import PoseEngine, make_ggs_cfg
from posediffusion_amd.host import denoiser_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5
LANE, NOLANE = _lib.PD_GGS_CFG_LANE_ITEMS, _lib.PD_GGS_CFG_NO_LANE_ITEMS
ONE_HOP, SPREAD = _lib.PD_GGS_CFG_FORCE_ONE_HOP, _lib.PD_GGS_CFG_XCHG_SPREAD
FLAGS = {"lane": LANE, "nolane": NOLANE, "one_hop": ONE_HOP, "spread": SPREAD}
WGS = (1, 0, 3, 17)

GGS_CASES = {                 # frames, matches per pair, both orders of every pair, scene seed
    "n2_x200": (2, 200, False, 7),          # (a scene whose start point keeps > 10 valid matches per frame)
    "n24_x30": (24, 30, False, 824),
    "n25_x30": (25, 30, False, 825),
    "n32_x16": (32, 16, False, 832),
    "n33_x16": (33, 16, False, 833),
    "n64_x8": (64, 8, False, 864),
    "n64_x5_ordered": (64, 5, True, 865),
}
# the kernel family pd_debug_ggs_plan reports at B = 1, per reserved flag, for wgs_per_seq = 1, 0, 3, 17 (WGS) on a 256-CU chip:
# lane = pd_ggs_lane_kernel; wave_k1_Ww = one workgroup of W waves; one_hop_kK / two_hop_kK = K workgroups on the single-exchange / two-hop
# kernel; refused = PD_ERR_UNSUPPORTED "LDS per workgroup" (64 frames: the one-hop kernel and too few two-hop workgroups cannot hold the items)
_UP_TO_32 = lambda k1, k0: [k1, k0, "one_hop_k3", "one_hop_k17"]
_TWO_HOP = lambda k0: ["refused", k0, "refused", "two_hop_k17"]
EXPECTED = {
    "n2_x200": dict(lane=["lane"] * 4, nolane=_UP_TO_32("wave_k1_8w", "wave_k1_8w"), one_hop=_UP_TO_32("wave_k1_8w", "wave_k1_8w"),
                    spread=_UP_TO_32("wave_k1_8w", "wave_k1_8w")),
    "n24_x30": {f: _UP_TO_32("wave_k1_12w", "one_hop_k35") for f in FLAGS},          # (the lane kernel's LDS image does not fit 276 pairs)
    "n25_x30": {f: _UP_TO_32("wave_k1_12w", "one_hop_k38") for f in FLAGS},
    "n32_x16": {f: _UP_TO_32("wave_k1_8w", "one_hop_k62") for f in FLAGS},
    "n33_x16": dict({f: ["wave_k1_8w", "two_hop_k66", "two_hop_k3", "two_hop_k17"] for f in FLAGS}, one_hop=_UP_TO_32("wave_k1_8w", "one_hop_k66")),
    "n64_x8": dict({f: _TWO_HOP("two_hop_k252") for f in FLAGS}, one_hop=["refused"] * 4),
    "n64_x5_ordered": dict({f: _TWO_HOP("two_hop_k256") for f in FLAGS}, one_hop=["refused"] * 4),
}


@pytest.fixture(scope="module")
def eng64(seeded_diffuser):
    dev = torch.device(DEV)
    diff = seeded_diffuser.to(dev)
    eng = PoseEngine(denoiser_state(diff.model), {k: v for k, v in diff.named_buffers(recurse=False)}, device=dev, max_B=80, max_N=64)
    yield eng
    eng.close()


def _family(eng, N, cfg):
    plan = (C.c_int * 8)()
    try:
        _lib.check(eng.lib.pd_debug_ggs_plan(eng._h, 1, N, C.byref(cfg), plan), "pd_debug_ggs_plan")
    except RuntimeError as e:
        assert "LDS per workgroup" in str(e), str(e)
        return "refused", None
    p = list(plan)
    if p[6]:
        return "lane", p
    if p[3]:
        return f"two_hop_k{p[0]}", p
    if p[0] > 1:
        return f"one_hop_k{p[0]}", p
    return f"wave_k1_{p[4]}w", p


@pytest.mark.parametrize("case", list(GGS_CASES))
def test_ggs_kernel_families_across_frame_counts_vs_fp64(eng64, case):
    N, per_pair, ordered, seed = GGS_CASES[case]
    enc = synth.make_cameras(N, seed=seed)
    md = synth.make_matches(enc, 224, 224, per_pair=per_pair, seed=seed, ordered_pairs=ordered)
    pairs = len(np.unique(md["i12"][:, 0] * N + md["i12"][:, 1]))
    assert pairs == (N * (N - 1) if ordered else N * (N - 1) // 2)
    eng64.set_matches(0, md["kp1"], md["kp2"], md["i12"], md["img_shape"])
    pm = O.prepare_matches(md["kp1"], md["kp2"], md["i12"], md["img_shape"])
    x0 = synth.perturb_pose(enc, seed=810 + N)
    ref64, s64 = oracle_optimize(x0, pm, iter_num=3)
    ref32, s32 = oracle_optimize(x0, pm, torch.float32, iter_num=3)
    assert s64 == s32 == 6
    families, worst, cache = {}, {}, {}
    for fname, flags in FLAGS.items():
        for wgs in WGS:
            tag = f"{case}/{fname}/k{wgs}"
            fam, plan = _family(eng64, N, make_ggs_cfg(wgs_per_seq=wgs, reserved=flags))
            families[(fname, wgs)] = fam
            assert fam == EXPECTED[case][fname][WGS.index(wgs)], (tag, fam, plan)
            if fam == "refused":
                with pytest.raises(RuntimeError, match="LDS per workgroup"):
                    eng64.ggs_loss_grad(x0.to(DEV), cfg=make_ggs_cfg(wgs_per_seq=wgs, reserved=flags))
                continue
            loss, grad = eng64.ggs_loss_grad(x0.to(DEV), cfg=make_ggs_cfg(wgs_per_seq=wgs, reserved=flags))
            eng64.check_async()
            eg, _ = check_loss_grad(loss[0].cpu(), grad.cpu(), x0, pm, tag, cache)
            out, st, _ = eng64.ggs_optimize(x0.to(DEV), cfg=make_ggs_cfg(iter_num=3, wgs_per_seq=wgs, reserved=flags))
            eng64.check_async()
            assert int(st[0, 1]) == s64, (tag, int(st[0, 1]))
            es, bnd = check_steps(out, x0, ref64, ref32, tag)
            w = worst.setdefault(fam, {"grad": {}, "step": {}})
            for g in eg:
                w["grad"][g] = max(w["grad"].get(g, 0.0), eg[g])
                w["step"][g] = max(w["step"].get(g, 0.0), es[g])
            w["step_bound"] = bnd
    print(f"\n{case}: {pairs} pairs; families {families}")
    for fam, w in worst.items():
        print(f"  {fam}: worst grad {({g: f'{v:.1e}' for g, v in w['grad'].items()})}, worst step {({g: f'{v:.1e}' for g, v in w['step'].items()})}, "
              f"step bound {({g: f'{v:.1e}' for g, v in w['step_bound'].items()})}")
    # one shortened geometry_guided_sampling (5 stages x 2 iterations; x 2 where all flags update): iterations per stage and the step
    cfg = dict(synth.GGS_CFG, iter_num=2)
    g, stg = eng64.ggs_guide(x0.to(DEV), 3, make_ggs_cfg(cfg))
    eng64.check_async()
    gd64, steps64 = oracle_guide(x0, md, cfg)
    gd32, _ = oracle_guide(x0, md, cfg, torch.float32)
    assert stg[0, :, 1].long().tolist() == steps64 == [4, 2, 2, 2, 4], (stg[0, :, 1].tolist(), steps64)
    es, bnd = check_steps(g, x0, gd64, gd32, f"{case}/guide")
    print(f"  guide (plan {_family(eng64, N, make_ggs_cfg(cfg))[0]}): step {({k: f'{v:.1e}' for k, v in es.items()})}, "
          f"bound {({k: f'{v:.1e}' for k, v in bnd.items()})}")


DENOISER_SHAPES = [(31, 33), (32, 33), (15, 64), (16, 64), (21, 50), (80, 64)]


@pytest.mark.parametrize("B,N", DENOISER_SHAPES)
def test_denoiser_above_32_frames_vs_fp64(eng64, oracle_weights, B, N):
    """Denoiser.forward at N > 32 on both sides of PD_STREAM_MIN_ROWS = 1 024 token rows: 1 023 / 1 056 rows at 33 frames, 960 / 1 024 at
    64, 1 050 at 50, and 5 120 rows at 64 frames (the 96-row strip tiles with pd_attn_seq_kernel).  Exact (0) and fp16-plane (2) modes
    against fp64, per sequence, with the rules of test_denoiser_at_the_bench_launch_shapes; the fused attention (pd_qkv_attn, N <= 32 only)
    forced on (PD_OPT_DENOISER_FUSED_ATTN = 2) must leave N > 32 bitwise on the two-launch path."""
    sd64 = {k: v.double() for k, v in oracle_weights.items()}
    g = torch.Generator().manual_seed(50 * B + N)
    x, z = torch.randn(B, N, 9, generator=g), synth.make_z(B, N, seed=B + 11)
    rows = B * N
    sub = {0, 1, B // 2, B - 1}
    for r in range(0, rows, 2048):
        sub.add(min(B - 1, (r + 1024) // N))
        sub.add(min(B - 1, r // N))
        sub.add(max(0, r // N - 1))
    sub = sorted(sub)
    res = {}
    try:
        for t in (99, 31, 0):
            with torch.no_grad():
                ref = O.denoiser_forward(sd64, x[sub].double(), torch.full((len(sub),), t, dtype=torch.long), z[sub].double())
            for mode in (0, 2):
                eng64.set_split_precision(mode)
                out = eng64.denoise(x.to(DEV), z.to(DEV), t)
                assert torch.isfinite(out).all()
                res[(t, mode)] = max(rel_err(out[s], ref[i]) for i, s in enumerate(sub))
        eng64.set_split_precision(2)
        for t in (99, 0):
            eng64.set_option(_lib.PD_OPT_DENOISER_FUSED_ATTN, 2)
            fused = eng64.denoise(x.to(DEV), z.to(DEV), t)
            eng64.set_option(_lib.PD_OPT_DENOISER_FUSED_ATTN, 0)
            plain = eng64.denoise(x.to(DEV), z.to(DEV), t)
            assert torch.equal(fused, plain), (B, N, t)
    finally:
        eng64.set_option(_lib.PD_OPT_DENOISER_FUSED_ATTN, 1)
        eng64.set_split_precision(2)
    print(f"B = {B}, N = {N} ({rows} rows), sequences {sub}: (t, mode) -> worst per-sequence rel. error vs fp64:",
          {k: f"{v:.2e}" for k, v in res.items()})
    for t in (99, 31, 0):
        assert res[(t, 0)] < TOL, (t, res)
        assert res[(t, 2)] <= max(2.0 * res[(t, 0)], 2e-6), (t, res)


def test_guided_sampling_n64_graph_replay_equals_eager(eng64):
    """pd_sample with GGS at N = 64 (2 016 pairs, 4 chunks: the two-hop kernel by default), B = 2: replayed from its hipGraph it equals
    eager launches bit for bit, and every pose and statistic is finite."""
    B, N = 2, 64
    for b in range(B):
        enc = synth.make_cameras(N, seed=900 + b)
        md = synth.make_matches(enc, 224, 224, per_pair=8, seed=900 + b)
        eng64.set_matches(b, md["kp1"], md["kp2"], md["i12"], md["img_shape"])
    z = synth.make_z(B, N, seed=21).to(DEV)
    noise = torch.randn(101, B, N, 9, generator=torch.Generator().manual_seed(22)).to(DEV)
    cfg = dict(synth.GGS_CFG, iter_num=5)
    pose_g, proc_g, st_g = eng64.sample(z, noise, 2, cfg, use_graph=True)
    pose_e, proc_e, st_e = eng64.sample(z, noise, 2, cfg, use_graph=False)
    eng64.check_async()
    assert torch.isfinite(pose_g).all() and torch.isfinite(proc_g).all()
    assert torch.equal(pose_g, pose_e) and torch.equal(proc_g, proc_e)
    assert torch.equal(st_g.nan_to_num(-1.0), st_e.nan_to_num(-1.0))
