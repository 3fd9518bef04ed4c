"""GPU (-m gpu), round 4 ("Next round" item 1 + ADVICE): the denoiser against the fp64 oracle AT THE BENCH'S OWN
LAUNCH SHAPES (5 120 / 2 560 / 2 060 token rows: the `b < full` block mapping of pd_gemm_strip_kernel / pd_gemm_dma_kernel and
pd_attn_mma_kernel at 1 024 workgroups), adversarial operands for the fp16-plane default, the fp16-subnormal behaviour of the
matrix pipe, the exchange-region guard of pd_ggs_plan and the kernel the engine picks by itself.  Everything goes through the C-ABI.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import pd_oracle as O
from posediffusion_amd import _lib, synth
from posediffusion_amd.engine import PoseEngine, make_ggs_cfg
from posediffusion_amd.host import denoiser_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5          # asserted teacher-forced bound (contract 1e-4 relative, BASELINE.json north_star)


def _engine(diff, B, N):
    dev = torch.device(DEV)
    diff = diff.to(dev)
    return PoseEngine(denoiser_state(diff.model), {k: v for k, v in diff.named_buffers(recurse=False)}, device=dev, max_B=B, max_N=N)


@pytest.mark.parametrize("B,N", [(256, 20), (128, 20), (103, 20)])
def test_denoiser_at_the_bench_launch_shapes(seeded_diffuser, oracle_weights, B, N):
    """Denoiser.forward (models/denoiser.py:53-98) at 256 x 20 = 5 120 rows (bench.py's engine pass: two full groups of 32 row tiles +
    a rest), 128 x 20 = 2 560 (one full group + 8 tiles) and 103 x 20 = 2 060 (ragged: 32 tiles + 12 rows), in the default fp16-plane
    mode and in the exact-fp32 mode, against the fp64 oracle.  Compared sequences: {0, 1, B/2, B-1} plus one sequence inside every
    2 048-row group and the sequences that straddle a group boundary."""
    eng = _engine(seeded_diffuser, B, N)
    sd64 = {k: v.double() for k, v in oracle_weights.items()}
    g = torch.Generator().manual_seed(40 * B + N)
    x, z = torch.randn(B, N, 9, generator=g), synth.make_z(B, N, seed=B + 7)
    rows = B * N
    sub = {0, 1, B // 2, B - 1}
    for r in range(0, rows, 2048):                      # a sequence inside each group, and the ones around each group boundary
        sub.add(min(B - 1, (r + 1024) // N))
        sub.add(min(B - 1, r // N))
        sub.add(max(0, r // N - 1))
    sub = sorted(sub)
    res = {}
    for t in (99, 31, 0):
        with torch.no_grad():
            ref = O.denoiser_forward(sd64, x[sub].double(), torch.full((len(sub),), t, dtype=torch.long), z[sub].double())
        for mode in (0, 2):
            eng.set_split_precision(mode)
            out = eng.denoise(x.to(DEV), z.to(DEV), t)
            assert torch.isfinite(out).all()
            res[(t, mode)] = max(rel_err(out[s], ref[i]) for i, s in enumerate(sub))     # worst sequence, each against its own scale
    print(f"B = {B}, N = {N} ({rows} rows), sequences {sub}: (t, mode) -> worst per-sequence rel. error vs fp64:",
          {k: f"{v:.2e}" for k, v in res.items()})
    for t in (99, 31, 0):
        assert res[(t, 0)] < TOL, (t, res)
        assert res[(t, 2)] <= max(2.0 * res[(t, 0)], 2e-6), (t, res)
    # the whole batch: both modes agree everywhere (no row tile of the launch is left out of the comparison above by accident)
    eng.set_split_precision(0)
    o0 = eng.denoise(x.to(DEV), z.to(DEV), 31)
    eng.set_split_precision(2)
    o2 = eng.denoise(x.to(DEV), z.to(DEV), 31)
    per_seq = ((o2 - o0).abs().amax(dim=(1, 2)) / o0.abs().amax(dim=(1, 2))).cpu()
    print(f"  default vs exact mode over all {B} sequences: worst {per_seq.max():.2e} at sequence {int(per_seq.argmax())}")
    assert per_seq.max() < 1e-5
    eng.close()


def _adversarial_state(diff, kind):
    """Encoder weights / biases outside the trunc-normal sigma = 0.02 family the round-3 test used."""
    sd = {k: v.detach().cpu().clone() for k, v in denoiser_state(diff.model).items()}
    g = torch.Generator().manual_seed(11)
    enc = [k for k in sd if "_trunk" in k and k.endswith(("in_proj_weight", "out_proj.weight", "linear1.weight", "linear2.weight"))]
    if kind == "outlier_weight_per_row":            # one weight per row at 100 sigma: max|w| pushes the bulk 2^-7 down the weight scale
        for k in enc:
            w = sd[k]
            col = torch.randint(0, w.shape[1], (w.shape[0],), generator=g)
            sgn = torch.where(torch.rand(w.shape[0], generator=g) < 0.5, -1.0, 1.0)
            w[torch.arange(w.shape[0]), col] = 2.0 * sgn
    elif kind == "bias_30x_activation":             # row bounds 30 x the typical activation: the operand scale leaves the values low in range
        for k in list(sd):
            if "_trunk" in k and k.endswith(("in_proj_bias", "linear1.bias")):
                b = sd[k]
                b[::2] = 30.0 * 0.45 * torch.where(torch.rand(b[::2].shape, generator=g) < 0.5, -1.0, 1.0)
    elif kind == "one_hot_layernorm_rows":          # x^ = +-sqrt(512) e_k (residual stream concentrated on one channel via _first.bias)
        sd["_first.bias"][137] = 3.0e4
    elif kind == "tiny_relu_outputs":               # ... and FF1 rows of alternating sign that cancel on it: ReLU outputs ~2^-20 of their bound
        sd["_first.bias"][137] = 1.0e6
        for k in list(sd):
            if "_trunk" in k and k.endswith("linear1.weight"):
                w = sd[k]
                alt = torch.where(torch.arange(w.shape[1]) % 2 == 0, 0.02, -0.02)
                w[:] = alt[None, :] * torch.where(torch.rand(w.shape[0], 1, generator=g) < 0.5, -1.0, 1.0)
                w[:, 137] = 0.0
            if "_trunk" in k and k.endswith("linear1.bias"):
                sd[k][:] = 1e-7
    else:
        raise KeyError(kind)
    return sd


@pytest.mark.parametrize("kind", ["outlier_weight_per_row", "bias_30x_activation", "one_hot_layernorm_rows", "tiny_relu_outputs"])
def test_fp16_plane_mode_under_adversarial_operands(seeded_diffuser, kind):
    """PD_OPT_DENOISER_SPLIT = 2 (the default at >= 1 024 token rows) rests on static power-of-two operand scales derived from bounds
    (pd_plane_exponents): here the bounds are loose or the values sit far below them.  One step against the fp64 oracle at three
    timesteps, error within 2 x the exact-fp32 mode's (floor 2e-6), nothing non-finite."""
    dev = torch.device(DEV)
    diff = seeded_diffuser.to(dev)
    sd = _adversarial_state(diff, kind)
    B, N = 52, 20
    eng = PoseEngine(sd, {k: v for k, v in diff.named_buffers(recurse=False)}, device=dev, max_B=B, max_N=N)
    sd64 = {k: v.double() for k, v in sd.items()}
    g = torch.Generator().manual_seed(3)
    x, z = torch.randn(B, N, 9, generator=g), synth.make_z(B, N, seed=5)
    sub = [0, 17, B - 1]
    rows = {}
    for t in (99, 40, 0):
        with torch.no_grad():
            ref = O.denoiser_forward(sd64, x[sub].double(), torch.full((len(sub),), t, dtype=torch.long), z[sub].double())
        e = {}
        for mode in (0, 2):
            eng.set_split_precision(mode)
            out = eng.denoise(x.to(dev), z.to(dev), t)
            assert torch.isfinite(out).all(), (kind, t, mode)
            e[mode] = rel_err(out[sub], ref)
        rows[t] = (e[0], e[2])
    print(f"{kind}: t -> (exact fp32 MFMA, fp16 planes) vs fp64:", {t: f"{a:.2e} {b:.2e}" for t, (a, b) in rows.items()})
    for t, (e0, e2) in rows.items():
        assert e0 < 1e-4 and e2 <= max(2.0 * e0, 2e-6), (kind, t, e0, e2)
    eng.close()


def test_fp16_matrix_pipe_keeps_subnormal_operands():
    """The `lo` halves of small elements are fp16 SUBNORMALS (|value x scale| < 2^-3): v_mfma_f32_32x32x16_f16 must not flush them, or
    those elements would keep 11 bits instead of 22.  pd_debug_mfma_f16_subnormal multiplies constant matrices: 16 x 2^-20 x 2^10 = 2^-6
    when kept, 0 when flushed (either operand), and a subnormal x normal product far below fp16's range (fp32 accumulation)."""
    lib = _lib.load()
    out = (C.c_float * 4)()
    with torch.cuda.device(DEV):
        _lib.check(lib.pd_debug_mfma_f16_subnormal(out, torch.cuda.current_stream().cuda_stream), "pd_debug_mfma_f16_subnormal")
    got = list(out)
    print("v_mfma_f32_32x32x16_f16 with fp16-subnormal operands (A sub, B sub, sub x 2^-4, control):", got)
    assert got[3] == 16.0
    assert got[0] == 2.0 ** -6 and got[1] == 2.0 ** -6, "the fp16 matrix pipe flushes subnormal operands: the lo plane needs its own scale"
    assert got[2] == 16.0 * 2.0 ** -24


def test_fp16_plane_mode_refuses_non_finite_weights(seeded_diffuser):
    """weights with inf / NaN have no static bounds -- the engine stays on the exact-fp32 kernels (which propagate them
    like the reference) and an explicit request for the mode fails with a message instead of undefined scales."""
    dev = torch.device(DEV)
    diff = seeded_diffuser.to(dev)
    sd = {k: v.detach().clone() for k, v in denoiser_state(diff.model).items()}
    sd["_trunk.layers.3.linear1.weight"][5, 7] = float("inf")
    eng = PoseEngine(sd, {k: v for k, v in diff.named_buffers(recurse=False)}, device=dev, max_B=52, max_N=20)
    with pytest.raises(RuntimeError, match="non-finite"):
        eng.set_split_precision(2)
    out = eng.denoise(torch.randn(52, 20, 9, device=dev), synth.make_z(52, 20, seed=1).to(dev), 10)    # exact mode: runs, propagates
    assert not torch.isfinite(out).all()
    eng.close()


def test_ggs_plan_keeps_the_exchange_region(seeded_diffuser):
    """with k > 1 every work item owns one exchange line in the sequence's region of 2 max_N^2 + 512 lines;
    a sequence with MORE items (15 pairs x 20 000 matches = 600 items at max_N = 6: 584 lines) must run on one workgroup (no exchange)
    instead of writing past its region.  Value, valid count and gradient against the oracle."""
    eng = _engine(seeded_diffuser, 1, 6)
    N = 6
    enc = synth.make_cameras(N, seed=321)
    md = synth.make_matches(enc, 224, 224, per_pair=20000, seed=322)
    eng.set_matches(0, md["kp1"], md["kp2"], md["i12"], md["img_shape"])
    cfg = make_ggs_cfg(synth.GGS_CFG)
    plan = (C.c_int * 8)()
    _lib.check(eng.lib.pd_debug_ggs_plan(eng._h, 1, N, C.byref(cfg), plan), "pd_debug_ggs_plan")
    print("plan {k, slots, lds, two_hop, waves, stage_p, lane, lane_rl}:", list(plan))
    assert plan[0] == 1 and plan[3] == 0 and plan[1] >= 600
    x0 = synth.perturb_pose(enc, seed=9).to(DEV)
    loss, grad = eng.ggs_loss_grad(x0, cfg=cfg)
    eng.check_async()
    # the oracle in fp64: 20 000 matches per pair are more than an fp32 autograd sums to 1e-4 itself (its fp32 gradient is 1.9e-4 away)
    pm = O.prepare_matches(md["kp1"].astype(np.float32).astype(np.float64), md["kp2"].astype(np.float32).astype(np.float64), md["i12"], md["img_shape"])
    xo = x0.cpu().double().clone().requires_grad_(True)
    v, _ = O.compute_sampson_distance(xo, pm)
    (go,) = torch.autograd.grad(v.mean(), xo)
    assert abs(int(loss[0, 1]) - len(v)) <= 2                      # (the documented threshold rule: within 1e-4 of sampson_max)
    assert abs(loss[0, 0].item() - v.mean().item()) < 1e-4 * v.mean().item() and rel_err(grad, go) < 1e-4
    o3, st3, _ = eng.ggs_optimize(x0, cfg=make_ggs_cfg(iter_num=3))
    eng.check_async()
    ref3, _, steps = O.ggs_optimize(x0.cpu().double().clone(), pm, iter_num=3)
    assert steps == int(st3[0, 1]) and rel_err(o3, ref3) < 1e-4
    eng.close()


def test_engine_picks_the_lane_kernel_where_a_sequence_gets_one_workgroup(seeded_diffuser):
    """pd_ggs_plan's own choice: more sequences than half the CUs (one workgroup per sequence is all there is) ->
    the lane-per-item kernel, whether the sequences are fully resident (40 matches per pair) or stream through its LDS ring (300: the
    bench shape, where it is 10 - 14 % faster since round 4); fewer sequences -> several workgroups per sequence on the wave-per-item
    kernels, and an EXPLICIT workgroup count without PD_GGS_CFG_LANE_ITEMS always stays on those (bitwise independent of the count)."""
    B, N = 130, 20
    eng = _engine(seeded_diffuser, B, N)
    enc = synth.make_cameras(N, seed=77)
    plan = (C.c_int * 8)()
    got = {}
    for per_pair in (40, 300):
        md = synth.make_matches(enc, 224, 224, per_pair=per_pair, seed=78)
        for b in range(B):
            eng.set_matches(b, md["kp1"], md["kp2"], md["i12"], md["img_shape"])
        for tag, nb, cfg in (("auto", B, make_ggs_cfg(synth.GGS_CFG)), ("auto", 64, make_ggs_cfg(synth.GGS_CFG)),
                             ("wgs1", B, make_ggs_cfg(synth.GGS_CFG, wgs_per_seq=1)),
                             ("wgs1_lane", 64, make_ggs_cfg(synth.GGS_CFG, wgs_per_seq=1, reserved=_lib.PD_GGS_CFG_LANE_ITEMS))):
            _lib.check(eng.lib.pd_debug_ggs_plan(eng._h, nb, N, C.byref(cfg), plan), "pd_debug_ggs_plan")
            got[(per_pair, tag, nb)] = list(plan)
    print("plans {k, slots, lds, two_hop, waves, stage_p, lane, ring steps}:", got)
    for per_pair in (40, 300):
        assert got[(per_pair, "auto", B)][6] == 1 and got[(per_pair, "auto", B)][0] == 1
        assert got[(per_pair, "auto", 64)][6] == 0 and got[(per_pair, "auto", 64)][0] > 1
        assert got[(per_pair, "wgs1", B)][6] == 0 and got[(per_pair, "wgs1", B)][0] == 1
        assert got[(per_pair, "wgs1_lane", 64)][6] == 1
    assert got[(300, "wgs1", B)][4] == 12                          # the staged 12-wave kernel
    eng.close()


def test_xcd_local_exchange_equals_the_spread_one(seeded_diffuser):
    """Round 4: at more than one workgroup per sequence the block -> (sequence, workgroup) map keeps a sequence's workgroups on one XCD
    and, once the launch-time handshake on XCC_ID has confirmed it, the exchange stores are plain stores through the shared L2
    (pd_ggs_kernels.h, `xl`).  PD_GGS_CFG_XCHG_SPREAD restores round 3's map + agent-scope stores.  The exchange only transports the items' sums:
    the poses, iteration counts and statistics must agree bit for bit, for one sequence, for a count that is not a multiple of 8 (padded map)
    and for k in {3, 24}, over enough iterations that a stale line would show."""
    B, N = 11, 20
    eng = _engine(seeded_diffuser, B, N)
    x0s = []
    for b in range(B):
        enc = synth.make_cameras(N, seed=4100 + b)
        md = synth.make_matches(enc, 224, 224, per_pair=60 + 20 * (b % 3), seed=4100 + b)
        eng.set_matches(b, md["kp1"], md["kp2"], md["i12"], md["img_shape"])
        x0s.append(synth.perturb_pose(enc, seed=90 + b))
    x0 = torch.cat(x0s).to(DEV)
    plan = (C.c_int * 8)()
    for nb in (1, 5, B):
        for k in (3, 24):
            if nb * k > 256:
                continue
            outs = []
            for flags in (0, _lib.PD_GGS_CFG_XCHG_SPREAD):
                cfg = make_ggs_cfg(synth.GGS_CFG, iter_num=40, wgs_per_seq=k, reserved=flags | _lib.PD_GGS_CFG_NO_LANE_ITEMS)
                _lib.check(eng.lib.pd_debug_ggs_plan(eng._h, nb, N, C.byref(cfg), plan), "pd_debug_ggs_plan")
                assert plan[0] == k, list(plan)
                out, stats = eng.ggs_guide(x0[:nb], 3, cfg)
                eng.check_async()
                outs.append((out.clone(), stats.clone()))
            assert torch.equal(outs[0][0], outs[1][0]), (nb, k)
            assert torch.equal(outs[0][1], outs[1][1]), (nb, k)
            assert torch.isfinite(outs[0][0]).all()
    eng.close()


def test_free_running_ggs_on_full_size_on_the_lane_kernel(engine, golden):
    """SURVEY 8c's free-running criterion at the benchmark's real size (fixture guided_free_full: BASELINE configs[2] exactly -- N = 20,
    57 000 matches, 100 steps, the last 10 guided x 700 = 7 000 iterations -- through the UNMODIFIED reference in fp32 and the fp64
    oracle) for the kernel the throughput shape runs since round 4: pd_ggs_lane_kernel (8 waves, uneven cuts ordered by length, LDS
    ring).  tests/test_gpu_parity_r2.py holds the wave-per-item kernels to the same bounds on the same fixture.  Per seed: pose deviation
    from fp64 <= 2 x the reference-fp32's own (5.8e-4); final mean Sampson gap to fp64 <= max(1 %, 2 x the reference's own 27 %);
    hipGraph replay == eager, all 7 000 iterations run (_free_running_case asserts both)."""
    from test_gpu_parity_r2 import _free_running_case
    g = golden["guided_free_full"]
    cfg = dict(synth.GGS_CFG, wgs_per_seq=1, reserved=_lib.PD_GGS_CFG_LANE_ITEMS)
    plan = (C.c_int * 8)()
    dev, ref_dev, gap, ref_gap = _free_running_case(engine, g, 0, cfg)
    c = make_ggs_cfg(cfg)
    _lib.check(engine.lib.pd_debug_ggs_plan(engine._h, 1, 20, C.byref(c), plan), "pd_debug_ggs_plan")
    assert plan[6] == 1, list(plan)                                       # it WAS the lane kernel
    print(f"free-running GGS-on, configs[2] full size, lane-per-item kernel: engine vs fp64 {dev:.3e} (reference fp32 {ref_dev:.3e}); "
          f"final mean Sampson gap to fp64: engine {gap:.3%}, reference fp32 {ref_gap:.3%}")
    assert dev <= 2.0 * ref_dev, (dev, ref_dev)
    assert gap <= max(0.01, 2.0 * ref_gap), (gap, ref_gap)


def test_embedding_modules_called_piecewise(seeded_diffuser, oracle_weights):
    """Rows D2 / D3 outside the fused denoiser: the drop-in `util.embedding.TimeStepEmbedding` / `PoseEmbedding` modules called the way
    a user of the reference's modules may call them (util/embedding.py:28-37, :52-54) run pd_time_embedding / pd_pose_embedding --
    the device code the engine's time table and `_first` staging use.  Time embedding against the fp64 oracle; the harmonic embedding
    against the oracle in fp32 (the reference itself forms `x 2^k + pi/2` in fp32, so fp64 is not the reference there) at pose-sized and
    at large arguments, 9-d poses in [B, N, 9] and another width."""
    dev = torch.device(DEV)
    model = seeded_diffuser.to(dev).model
    sd64 = {k: v.double() for k, v in oracle_weights.items()}
    for t in (torch.tensor([0, 1, 7, 42, 99], device=dev), torch.arange(100, device=dev), torch.tensor([3], device=dev, dtype=torch.int32)):
        out = model.time_embed(t)
        ref = O.timestep_embedding(t.cpu().long(), sd64)
        assert out.shape == (t.shape[0], 128) and out.dtype == torch.float32
        assert rel_err(out, ref) < 5e-6, rel_err(out, ref)          # an fp32 fmaf chain of 256 + 128 terms (6e-7 expected)
    assert model.time_embed(torch.zeros(0, dtype=torch.long, device=dev)).shape == (0, 128)
    g = torch.Generator().manual_seed(11)
    for shape, scale in (((2, 5, 9), 1.0), ((3, 20, 9), 30.0), ((7, 4), 1.0), ((1, 9), 1e-3)):
        x = (scale * torch.randn(*shape, generator=g)).float()
        out = model.pose_embed(x.to(dev))
        ref = O.harmonic_embedding(x)
        assert out.shape == ref.shape == (*shape[:-1], 21 * shape[-1])
        assert (out.cpu() - ref).abs().max().item() < 2e-6, (shape, scale, (out.cpu() - ref).abs().max().item())
        assert torch.equal(out[..., -shape[-1]:].cpu(), x)                       # append_input: the input itself, bit for bit
    assert model.pose_embed(torch.zeros(0, 9, device=dev)).shape == (0, 189)
    assert model.pose_embed.out_dim == 189 and model.time_embed.out_dim == 128
    with pytest.raises(RuntimeError, match="only on an AMD GPU"):
        model.pose_embed(torch.zeros(1, 9))
    lib = _lib.load()
    assert lib.pd_pose_embedding(None, 1, 9, None, None) == -1 and "pd_pose_embedding" in _lib.last_error()      # PD_ERR_INVALID_ARG
    assert lib.pd_time_embedding(None, None, None, None, None, 1, None, None) == -1
