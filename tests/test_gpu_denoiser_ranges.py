"""GPU (-m gpu): the denoiser at the limits of its configuration family (include/pd_engine.h, pd_weights) against fp64.

  1. tests/denoiser_cfgs.py EDGE_CFGS on the shape-generic path (posediffusion_amd/csrc/pd_denoiser_generic.hip): denoise at
     (B, N) = (1, 1), (2, 64), (3, 33), (5, 13), (70, 31) and t = T-1, T/2, 0; the fused DDPM tail (p_mean, p_finish); objective pred_x0.
  2. pd_engine_create refuses every value just outside a limit with an error that names the limit (pd_denoiser_generic_shape_ok).
  3. Two generic engines of different shapes alive in one process (pd_gen_attn_kernel's dynamic-LDS limit is a per-process attribute).
  4. The default-shape kernels at 1 and 16 layers: small-batch and streamed paths, the fp16-plane and bf16 modes, and the generic path.
  5. Schedules of T = 1 and T = 1000: teacher-forced sample steps against the fp64 p_sample formulas, graph replay == eager.
Every comparison is per pose column group (conftest.pose_err) against an fp64 forward of the same weights.
"""
import ctypes as C

import pytest
import torch

from conftest import pose_err
from denoiser_cfgs import EDGE_CFGS, build_dropin, fp64_copy, fp64_forward
from oracle import pd_oracle as O
from posediffusion_amd import _lib, synth
from posediffusion_amd.engine import PoseEngine
from posediffusion_amd.host import denoiser_state
from posediffusion_amd.schedule import diffusion_buffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5
# (70, 31): 2 170 token rows -- the GEMM's remainder tiles, M % 4 != 0 in the row kernels, M % 64 != 0
SHAPES = [(1, 1), (2, 64), (3, 33), (5, 13), (70, 31)]


def _engine(den, max_B, max_N, tables=None, generic=False, objective="pred_noise"):
    layer = den._trunk.layers[0]
    return PoseEngine(denoiser_state(den), tables if tables is not None else diffusion_buffers(), device=torch.device(DEV), max_B=max_B,
                      max_N=max_N, num_layers=len(den._trunk.layers), nhead=layer.self_attn.num_heads, objective=objective,
                      norm_first=layer.norm_first, pivot=den.pivot_cam_onehot, generic=generic)


def _sub(B):
    return sorted({0, B // 2, B - 1})


def _tables64(T=100):
    return O.diffusion_tables(timesteps=T, dtype=torch.float64)


def _posterior64(tb, t, x, model_out, pred_x0=False):
    """(mean, x0) of p_mean_variance in fp64 (models/gaussian_diffuser.py:190-205, :221-246)."""
    x0 = model_out if pred_x0 else tb["sqrt_recip_alphas_cumprod"][t] * x - tb["sqrt_recipm1_alphas_cumprod"][t] * model_out
    return tb["posterior_mean_coef1"][t] * x0 + tb["posterior_mean_coef2"][t] * x, x0


def _p_sample64(tb, t, mean, noise):
    """p_sample's output (:278-280): no noise term at t = 0."""
    return mean + (torch.exp(0.5 * tb["posterior_log_variance_clipped"][t]) * noise.double() if t > 0 else 0.0)


def _inputs(B, N, zdim, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, 9, generator=g), torch.randn(B, N, zdim, generator=g)


# ------------------------------------------------------------------------------------------------ 1. edge configurations
@pytest.mark.parametrize("ci", range(len(EDGE_CFGS)), ids=[c.name for c in EDGE_CFGS])
def test_edge_cfg_denoise_and_tail_vs_fp64(ci):
    cfg = EDGE_CFGS[ci]
    den = build_dropin(cfg, seed=60 + ci)
    d64, tb = fp64_copy(den), _tables64()
    eng = _engine(den, 70, 64)
    errs = {}
    try:
        for B, N in SHAPES:
            x, z = _inputs(B, N, cfg.z, 1000 * B + N)
            sub = _sub(B)
            for t in (99, 50, 0):
                out = eng.denoise(x.to(DEV), z.to(DEV), t)
                assert torch.isfinite(out).all()
                ref = fp64_forward(d64, x[sub], torch.tensor([t]), z[sub])
                errs[("denoise", B, N, t)] = pose_err(out[sub], ref, tag=f"ranges/denoise/{cfg.name}")
        # the fused tail (pd_gen_tail_kernel): posterior mean and x0, then p_finish with noise
        B, N = 3, 33
        x, z = _inputs(B, N, cfg.z, 77)
        noise = torch.randn(B, N, 9, generator=torch.Generator().manual_seed(78))
        for t in (99, 0):
            mean, x0 = eng.p_mean(x.to(DEV), z.to(DEV), t)
            nxt = eng.p_finish(mean, noise.to(DEV), t)
            mean64, x064 = _posterior64(tb, t, x.double(), fp64_forward(d64, x, torch.tensor([t]), z))
            tag = f"ranges/tail/{cfg.name}"
            errs[("x0", t)] = pose_err(x0, x064, tag=tag)
            errs[("mean", t)] = pose_err(mean, mean64, tag=tag)
            errs[("p_finish", t)] = pose_err(nxt, _p_sample64(tb, t, mean64, noise), tag=tag)
        eng.check_async()
    finally:
        eng.close()
    print(cfg.name, "worst", f"{max(errs.values()):.2e}", {k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad


PRED_X0_CFGS = [c for c in EDGE_CFGS if c.hidden in (1, 1024)]


@pytest.mark.parametrize("cfg", PRED_X0_CFGS, ids=[c.name for c in PRED_X0_CFGS])
def test_edge_cfg_pred_x0_vs_fp64(cfg):
    """GaussianDiffusion(objective="pred_x0") on the generic path: the network output IS x_start (gaussian_diffuser.py:225-227)."""
    den = build_dropin(cfg, seed=90 + cfg.hidden)
    d64, tb = fp64_copy(den), _tables64()
    eng = _engine(den, 5, 13, objective="pred_x0")
    errs = {}
    try:
        B, N = 5, 13
        x, z = _inputs(B, N, cfg.z, 91)
        noise = torch.randn(B, N, 9, generator=torch.Generator().manual_seed(92))
        for t in (99, 50, 0):
            ref = fp64_forward(d64, x, torch.tensor([t]), z)
            mean64, x064 = _posterior64(tb, t, x.double(), ref, pred_x0=True)
            mean, x0 = eng.p_mean(x.to(DEV), z.to(DEV), t)
            tag = f"ranges/pred_x0/{cfg.name}"
            errs[("denoise", t)] = pose_err(eng.denoise(x.to(DEV), z.to(DEV), t), ref, tag=tag)
            errs[("x0", t)] = pose_err(x0, x064, tag=tag)
            errs[("mean", t)] = pose_err(mean, mean64, tag=tag)
            errs[("p_finish", t)] = pose_err(eng.p_finish(mean, noise.to(DEV), t), _p_sample64(tb, t, mean64, noise), tag=tag)
        eng.check_async()
    finally:
        eng.close()
    print(cfg.name, "pred_x0 worst", f"{max(errs.values()):.2e}")
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 2. the C-ABI's accepted range
def _hand_state_dict(d=64, ff=64, z=16, hidden=32, layers=1, pivot=True, t_emb=256):
    """Zeros in the reference's keys and shapes (consistent with each other, so that no refusal depends on a mismatched tensor)."""
    sd = {"time_embed.linear.0.weight": torch.zeros(128, t_emb), "time_embed.linear.0.bias": torch.zeros(128),
          "time_embed.linear.2.weight": torch.zeros(128, 128), "time_embed.linear.2.bias": torch.zeros(128),
          "_first.weight": torch.zeros(d, 189 + t_emb // 2 + z + int(pivot)), "_first.bias": torch.zeros(d),
          "_last.0.weight": torch.zeros(hidden, d), "_last.0.bias": torch.zeros(hidden), "_last.1.weight": torch.zeros(hidden),
          "_last.1.bias": torch.zeros(hidden), "_last.3.weight": torch.zeros(9, hidden), "_last.3.bias": torch.zeros(9)}
    for l in range(layers):
        p = f"_trunk.layers.{l}."
        sd.update({p + "norm1.weight": torch.zeros(d), p + "norm1.bias": torch.zeros(d), p + "norm2.weight": torch.zeros(d),
                   p + "norm2.bias": torch.zeros(d), p + "self_attn.in_proj_weight": torch.zeros(3 * d, d),
                   p + "self_attn.in_proj_bias": torch.zeros(3 * d), p + "self_attn.out_proj.weight": torch.zeros(d, d),
                   p + "self_attn.out_proj.bias": torch.zeros(d), p + "linear1.weight": torch.zeros(ff, d), p + "linear1.bias": torch.zeros(ff),
                   p + "linear2.weight": torch.zeros(d, ff), p + "linear2.bias": torch.zeros(d)})
    return sd


MSG_D = r"d_model must be a multiple of 32 in \[32, 2048\]"
MSG_HD = r"head dim d_model / nhead must be a multiple of 4 in \[8, 256\]"
MSG_FF = r"dim_feedforward must be in \[1, 8192\]"
MSG_Z = r"z_dim must be in \[1, 4096\]"
MSG_HID = r"mlp_hidden_dim must be in \[1, 1024\]"
MSG_LAYERS = r"num_encoder_layers must be in \[1, PD_MAX_LAYERS = 16\]"
MSG_EMB = r"10 harmonics, t_emb 256"
# (state-dict shape, nhead, pattern): one value just outside one limit each
OUTSIDE = [
    (dict(d=2080), 4, MSG_D),
    (dict(d=16), 2, MSG_D),
    (dict(d=32), 8, MSG_HD),            # head dim 4
    (dict(d=96), 16, MSG_HD),           # head dim 6
    (dict(d=1056), 4, MSG_HD),          # head dim 264
    (dict(ff=0), 4, MSG_FF),
    (dict(ff=8193), 4, MSG_FF),
    (dict(z=0), 4, MSG_Z),
    (dict(z=4097), 4, MSG_Z),
    (dict(hidden=0), 4, MSG_HID),
    (dict(hidden=1025), 4, MSG_HID),
    (dict(layers=0), 4, MSG_LAYERS),
    (dict(t_emb=254), 4, MSG_EMB),
]


@pytest.mark.parametrize("shape,nhead,msg", OUTSIDE, ids=[f"{k}={v}" for s, _, _ in OUTSIDE for k, v in s.items()])
def test_engine_refuses_configuration_outside_the_family(shape, nhead, msg):
    """PoseEngine from a hand-made state dict: the drop-in's ValueError is not in the way, pd_denoiser_generic_shape_ok itself refuses."""
    layers = shape.get("layers", 1)
    sd = _hand_state_dict(**dict(shape, layers=max(layers, 1)))      # PoseEngine reads dim_ff from layer 0's linear1 even at 0 layers
    with pytest.raises(RuntimeError, match=msg):
        PoseEngine(sd, diffusion_buffers(), device=torch.device(DEV), max_B=2, max_N=4, num_layers=layers, nhead=nhead)


@pytest.mark.parametrize("over,msg", [(dict(num_layers=17), MSG_LAYERS), (dict(n_harmonic=9), MSG_EMB), (dict(n_harmonic=11), MSG_EMB)],
                         ids=["num_layers=17", "n_harmonic=9", "n_harmonic=11"])
def test_engine_refuses_what_pose_engine_cannot_express(over, msg):
    """pd_weights filled directly (17 layers do not fit its 16 layer slots; PoseEngine always passes 10 harmonics).  Every weight
    pointer is NULL: the shape check refuses before any of them is read, and a creation that got past it would fail on the NULL."""
    lib = _lib.load()
    tables = {k: v.to(DEV).contiguous() for k, v in diffusion_buffers().items()}
    w = _lib.pd_weights()
    w.d_model, w.nhead, w.dim_ff, w.num_layers, w.z_dim, w.n_harmonic = 64, 4, 64, 1, 16, 10
    w.t_emb_dim, w.mlp_hidden, w.timesteps = 256, 32, 100
    for name in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
                 "posterior_log_variance_clipped"):
        setattr(w, name, tables[name].data_ptr())
    for k, v in over.items():
        setattr(w, k, v)
    h = C.c_void_p(None)
    torch.cuda.synchronize()
    rc = lib.pd_engine_create(C.byref(w), 2, 4, C.byref(h))
    if rc == 0:
        lib.pd_engine_destroy(h)
    assert rc != 0 and not h.value
    with pytest.raises(RuntimeError, match=msg):
        _lib.check(rc, "pd_engine_create")


# ------------------------------------------------------------------------------------------------ 3. two generic engines in one process
def test_two_generic_engines_of_different_shapes():
    """Engine A (head dim 256, max_N 64, created first) and engine B (head dim 8, max_N 2) alive together, denoise calls interleaved, then
    A alone after B is destroyed.  pd_gen_attn_kernel's dynamic-LDS limit belongs to the process: B's creation must not lower it below
    what A's launches at N = 64 use (2 x 64 x 260 x 4 = 133 120 bytes)."""
    ca, cb = EDGE_CFGS[4], EDGE_CFGS[0]
    assert ca.d // ca.heads == 256 and cb.d // cb.heads == 8
    den_a, den_b = build_dropin(ca, seed=31), build_dropin(cb, seed=32)
    xa, za = _inputs(2, 64, ca.z, 33)
    xb, zb = _inputs(3, 2, cb.z, 34)
    ref_a = {t: fp64_forward(den_a, xa, torch.tensor([t]), za) for t in (99, 7)}
    ref_b = {t: fp64_forward(den_b, xb, torch.tensor([t]), zb) for t in (99, 7)}
    a = _engine(den_a, 2, 64)
    errs = {}
    try:
        b = _engine(den_b, 3, 2)
        try:
            for rep in range(2):
                for t in (99, 7):
                    errs[("A", rep, t)] = pose_err(a.denoise(xa.to(DEV), za.to(DEV), t), ref_a[t], tag="ranges/two_engines")
                    errs[("B", rep, t)] = pose_err(b.denoise(xb.to(DEV), zb.to(DEV), t), ref_b[t], tag="ranges/two_engines")
            b.check_async()
        finally:
            b.close()
        for t in (99, 7):
            errs[("A after B", t)] = pose_err(a.denoise(xa.to(DEV), za.to(DEV), t), ref_a[t], tag="ranges/two_engines")
        a.check_async()
    finally:
        a.close()
    print("two engines worst", f"{max(errs.values()):.2e}")
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 4. the default shape at 1 and 16 layers
@pytest.mark.parametrize("L", [1, 16])
def test_default_shape_layer_count_vs_fp64(L):
    """pd_denoiser_default_shape sends every num_layers in [1, 16] at the default shape to the specialised kernels (PdPlaneExps
    e[PD_MAX_LAYERS] included).  Exact fp32 below 1 024 rows and on the streamed path (52 x 20 rows): TOL; the fp16-plane mode (split 2):
    2 x the exact mode's error, as test_fp16_plane_denoiser_mode_is_fp32_grade; the bf16 fast mode (split 1): its 1e-4 contract; the
    generic kernels at the same weights (PD_WEIGHTS_GENERIC): TOL."""
    diff = synth.make_diffuser(seed=20 + L, num_layers=L)
    synth.randomize_norm_and_bias_(diff.model)
    den = diff.model.eval()
    sd64 = O.cast_state_dict(den.state_dict(), torch.float64)

    def ref(x, z, t):
        with torch.no_grad():
            return O.denoiser_forward(sd64, x.double(), torch.full((x.shape[0],), t, dtype=torch.long), z.double(), num_layers=L)

    tag = f"ranges/default_shape_L{L}"
    errs, split = {}, {}
    eng = _engine(den, 52, 33)
    gen = _engine(den, 52, 33, generic=True)
    try:
        assert eng.get_option(_lib.PD_OPT_DENOISER_SPLIT) == 2 and gen.get_option(_lib.PD_OPT_DENOISER_SPLIT) == 0
        for B, N in ((1, 1), (3, 33), (31, 33), (52, 20)):            # 31 x 33 = 1 023 rows: the last below the streamed path
            x, z = torch.randn(B, N, 9, generator=torch.Generator().manual_seed(B * 64 + N)), synth.make_z(B, N, seed=5 * B + N)
            sub = _sub(B)
            for t in (99, 40, 0):
                r = ref(x[sub], z[sub], t)
                eng.set_split_precision(0)
                errs[("exact", B, N, t)] = pose_err(eng.denoise(x.to(DEV), z.to(DEV), t)[sub], r, tag=tag)
                errs[("generic", B, N, t)] = pose_err(gen.denoise(x.to(DEV), z.to(DEV), t)[sub], r, tag=tag + "/generic")
                if B * N >= 1024:
                    for mode in (2, 1):
                        eng.set_split_precision(mode)
                        split[(mode, t)] = pose_err(eng.denoise(x.to(DEV), z.to(DEV), t)[sub], r, tag=f"{tag}/split{mode}")
                    split[(0, t)] = errs[("exact", B, N, t)]
        eng.check_async()
        gen.check_async()
    finally:
        eng.close()
        gen.close()
    print(f"L={L} exact/generic worst {max(errs.values()):.2e}; split modes", {k: f"{v:.1e}" for k, v in split.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad
    for t in (99, 40, 0):
        assert split[(2, t)] <= max(2.0 * split[(0, t)], 1e-6), (t, split)
        assert split[(1, t)] < 1e-4, (t, split)


# ------------------------------------------------------------------------------------------------ 5. schedules other than T = 100
@pytest.mark.parametrize("T", [1, 1000])
@pytest.mark.parametrize("which", ["default", "edge"])
def test_schedule_length_teacher_forced_and_graph(which, T):
    """pd_engine_create accepts 1 <= timesteps <= 4096.  Teacher-forced sample steps (first, middle, last) against the fp64 p_sample
    formulas with O.diffusion_tables(timesteps=T); graph replay equals eager execution bit for bit.  At T = 1 the one step has t = 0:
    the output is the posterior mean, without noise."""
    if which == "default":
        diff = synth.make_diffuser(seed=0)
        synth.randomize_norm_and_bias_(diff.model)
        den = diff.model.eval()
        sd64 = O.cast_state_dict(den.state_dict(), torch.float64)

        def forward64(x, t, z):
            with torch.no_grad():
                return O.denoiser_forward(sd64, x, torch.full((x.shape[0],), t, dtype=torch.long), z.double())
    else:
        den = build_dropin(EDGE_CFGS[1], seed=55)
        d64 = fp64_copy(den)

        def forward64(x, t, z):
            return fp64_forward(d64, x, torch.tensor([t]), z)
    zdim = den._first.in_features - 317 - int(den.pivot_cam_onehot)
    B, N = 2, 20
    tables, tb = diffusion_buffers(timesteps=T), _tables64(T)
    eng = _engine(den, B, N, tables=tables)
    try:
        assert eng.timesteps == T
        z = torch.randn(B, N, zdim, generator=torch.Generator().manual_seed(T))
        noise = torch.randn(T + 1, B, N, 9, generator=torch.Generator().manual_seed(T + 1))
        pose, process, _ = eng.sample(z.to(DEV), noise.to(DEV), 0, None, use_graph=False)
        pose_g, process_g, _ = eng.sample(z.to(DEV), noise.to(DEV), 0, None, use_graph=True)
        eng.check_async()
    finally:
        eng.close()
    assert torch.equal(pose_g, pose) and torch.equal(process_g, process)
    process = process.cpu()
    assert process.shape[0] == T + 1 and torch.equal(pose.cpu(), process[T]) and torch.equal(process[0], noise[0])
    errs = {}
    for step in sorted({0, T // 2, T - 1}):
        t = T - 1 - step
        x = process[step].double()
        mean64, _ = _posterior64(tb, t, x, forward64(x, t, z))
        errs[(step, t)] = pose_err(process[step + 1], _p_sample64(tb, t, mean64, noise[step + 1]), tag=f"ranges/schedule_T{T}/{which}")
    print(which, f"T={T}", {k: f"{v:.1e}" for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad
