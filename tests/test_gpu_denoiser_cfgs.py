"""GPU (-m gpu): non-default Denoiser configurations on the shape-generic denoiser path (posediffusion_amd/csrc/pd_denoiser_generic.hip).

  * Five configurations (sizes, post-norm, no pivot, a 2 048-wide z) at (B, N) = (1, 1), (1, 64), (5, 13), (256, 20) against the fp64
    forward of tests/denoiser_cfgs.py, per column group (pose_err).
  * The reference's own outputs for three configurations (tests/golden/denoiser_cfgs.npz, tools/make_denoiser_cfg_golden.py).
  * PD_WEIGHTS_GENERIC: the generic kernels at the default shape against tests/golden/denoiser.npz.
  * Sampling on a generic engine: teacher-forced steps against fp64, graph replay == eager, a guided batch, the pipeline's gated phases.
  * Options of a generic engine; PoseDiffusionModel.forward with a non-default DENOISER.TRANSFORMER.
"""
import pytest
import torch

from conftest import load_golden, pose_err
from denoiser_cfgs import CONFIGS, GOLDEN_CFGS, Cfg, build_dropin, fp64_forward, weight_checksum
from posediffusion_amd import _lib, synth
from posediffusion_amd.engine import PoseEngine, make_ggs_cfg
from posediffusion_amd.host import denoiser_state, draw_noise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5
SHAPES = [(1, 1), (1, 64), (5, 13), (256, 20)]


def _tables():
    from posediffusion_amd.schedule import diffusion_buffers
    return diffusion_buffers()


def _engine(den, max_B, max_N, generic=False, tables=None):
    return PoseEngine(denoiser_state(den), tables or _tables(), device=torch.device(DEV), max_B=max_B, max_N=max_N,
                      num_layers=len(den._trunk.layers), nhead=den._trunk.layers[0].self_attn.num_heads,
                      norm_first=den._trunk.layers[0].norm_first, pivot=den.pivot_cam_onehot, generic=generic)


def _sub(B):
    return sorted({0, B // 2, B - 1})


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c.name for c in CONFIGS])
def test_generic_denoiser_vs_fp64(cfg):
    den = build_dropin(cfg, seed=40 + cfg.d)
    eng = _engine(den, 256, 64)
    try:
        assert eng.get_option(_lib.PD_OPT_DENOISER_SPLIT) == 0
        errs = {}
        for B, N in SHAPES:
            g = torch.Generator().manual_seed(B * 100 + N)
            x, z = torch.randn(B, N, 9, generator=g), torch.randn(B, N, cfg.z, generator=g)
            sub = _sub(B)
            for t in (99, 4):
                out = eng.denoise(x.to(DEV), z.to(DEV), t)
                assert torch.isfinite(out).all()
                ref = fp64_forward(den, x[sub], torch.tensor([t]), z[sub])
                errs[(B, N, t)] = pose_err(out[sub], ref, tag=f"generic/{cfg.name}")
        print(cfg.name, {k: f"{v:.1e}" for k, v in errs.items()})
        assert max(errs.values()) < TOL, errs
    finally:
        eng.close()


def test_generic_denoiser_vs_reference_fixture():
    gold = load_golden("denoiser_cfgs.npz")
    for ci, cfg in enumerate(GOLDEN_CFGS):
        c = gold[f"c{ci}_cfg"].tolist()
        assert Cfg(*c[:6], bool(c[6]), bool(c[7])) == cfg
        den = build_dropin(cfg, seed=int(c[8]))
        assert weight_checksum(den.state_dict(), cfg.layers) == pytest.approx(gold[f"c{ci}_weight_checksum"], rel=1e-9)
        eng = _engine(den, 3, 9)
        try:
            for name in ("b2n5", "b1n1", "b3n9"):
                x, z = torch.from_numpy(gold[f"c{ci}_{name}_x"]), torch.from_numpy(gold[f"c{ci}_{name}_z"])
                for t in (99, 3):
                    out = eng.denoise(x.to(DEV), z.to(DEV), t)
                    e = pose_err(out, torch.from_numpy(gold[f"c{ci}_{name}_eps_t{t}"]), tag="generic/reference_fixture")
                    assert e < TOL, (cfg.name, name, t, e)
        finally:
            eng.close()


def test_generic_flag_at_default_shape_vs_reference_fixture(seeded_diffuser, golden):
    """PD_WEIGHTS_GENERIC: the generic kernels at cfgs/default.yaml's shape against the reference's own outputs (tests/golden/denoiser.npz)."""
    den = seeded_diffuser.model
    gold = golden["denoiser"]
    eng = _engine(den, 3, 33, generic=True)
    try:
        for name in ("b2n20", "b1n7", "b3n33"):
            x, z = torch.from_numpy(gold[f"{name}_x"]), torch.from_numpy(gold[f"{name}_z"])
            for t in (99, 50, 0):
                out = eng.denoise(x.to(DEV), z.to(DEV), t)
                e = pose_err(out, torch.from_numpy(gold[f"{name}_eps_t{t}"]), tag="generic/default_shape")
                assert e < TOL, (name, t, e)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def gen_engine():
    cfg = CONFIGS[0]
    den = build_dropin(cfg, seed=7)
    tables = _tables()
    eng = _engine(den, 5, 20, tables=tables)
    yield cfg, den, tables, eng
    eng.close()


def _matches(eng, B, N, seed):
    for b in range(B):
        enc = synth.make_cameras(N, seed=seed + b)
        md = synth.make_matches(enc, 224, 224, per_pair=40, seed=seed + b)
        eng.set_matches(b, md["kp1"], md["kp2"], md["i12"], md["img_shape"])


def test_generic_sampling_teacher_forced_vs_fp64(gen_engine):
    cfg, den, tables, eng = gen_engine
    B, N = 2, 20
    z = torch.randn(B, N, cfg.z, generator=torch.Generator().manual_seed(3))
    noise = torch.randn(101, B, N, 9, generator=torch.Generator().manual_seed(4))
    pose, process, _ = eng.sample(z.to(DEV), noise.to(DEV), 0, None, use_graph=False)
    eng.check_async()
    process = process.cpu()
    tb = {k: v.double().cpu() for k, v in tables.items()}
    for step in (0, 50, 90, 99):
        t = 99 - step
        x = process[step].double()
        eps = fp64_forward(den, x, torch.tensor([t]), z)
        x0 = tb["sqrt_recip_alphas_cumprod"][t] * x - tb["sqrt_recipm1_alphas_cumprod"][t] * eps
        mean = tb["posterior_mean_coef1"][t] * x0 + tb["posterior_mean_coef2"][t] * x
        nxt = mean + (torch.exp(0.5 * tb["posterior_log_variance_clipped"][t]) * noise[step + 1].double() if t > 0 else 0.0)
        e = pose_err(process[step + 1], nxt, tag="generic/p_sample")
        assert e < TOL, (step, e)
    assert torch.equal(pose.cpu(), process[100])


def test_generic_sampling_graph_equals_eager_and_guided(gen_engine):
    cfg, den, tables, eng = gen_engine
    B, N = 4, 20
    _matches(eng, B, N, 600)
    z = torch.randn(B, N, cfg.z, generator=torch.Generator().manual_seed(5)).to(DEV)
    noise = torch.randn(101, B, N, 9, generator=torch.Generator().manual_seed(6)).to(DEV)
    pg, prg, _ = eng.sample(z, noise, 0, None, use_graph=True)
    pe, pre, _ = eng.sample(z, noise, 0, None, use_graph=False)
    gcfg = dict(synth.GGS_CFG, iter_num=5)
    qg, qrg, sg = eng.sample(z, noise, 3, gcfg, use_graph=True)
    qe, qre, se = eng.sample(z, noise, 3, gcfg, use_graph=False)
    eng.check_async()
    assert torch.equal(pg, pe) and torch.equal(prg, pre)
    assert torch.equal(qg, qe) and torch.equal(qrg, qre) and torch.equal(sg.nan_to_num(-1.0), se.nan_to_num(-1.0))
    assert torch.isfinite(qg).all() and torch.isfinite(qrg).all()


def test_generic_pipeline_gated_phases_equal_whole_loop(gen_engine):
    from posediffusion_amd.pipeline import SamplingPipeline
    cfg, den, tables, eng0 = gen_engine
    dev = torch.device(DEV)
    B, N = 2, 12
    engs = [_engine(den, B, N, tables=tables) for _ in range(2)]
    try:
        data = []
        for e, eng in enumerate(engs):
            z = torch.randn(B, N, cfg.z, generator=torch.Generator().manual_seed(70 + e)).to(dev)
            noise = torch.stack([draw_noise((N, 9), 100, dev, 4, True, generator=torch.Generator(device=dev).manual_seed(80 + 10 * e + b))
                                 for b in range(B)], dim=1)
            _matches(eng, B, N, 700 + 10 * e)
            data.append((z, noise))
        gcfg = make_ggs_cfg(synth.GGS_CFG, iter_num=5, min_matches=0)
        torch.cuda.synchronize()
        refs = [tuple(v.clone() for v in engs[j].sample(data[j][0], data[j][1], 4, gcfg, use_graph=True)) for j in range(2)]
        torch.cuda.synchronize()
        pipe = SamplingPipeline(engs, 2, dev, unguided_streams=1)
        pend = []
        for _ in range(4):
            j = pipe.next_context()
            pend.append(pipe.submit(data[j][0], data[j][1], 4, gcfg, use_graph=True, want_process=True))
        pipe.synchronize()
        pipe.check_async()
        for p in pend:
            pose, proc, stats = p.wait()
            assert torch.equal(pose, refs[p.context][0]) and torch.equal(proc, refs[p.context][1])
            assert torch.equal(stats, refs[p.context][2])
    finally:
        for e in engs:
            e.close()


def test_generic_engine_options(gen_engine, seeded_diffuser):
    cfg, den, tables, eng = gen_engine
    assert eng.get_option(_lib.PD_OPT_DENOISER_SPLIT) == 0
    for mode in (1, 2):
        with pytest.raises(RuntimeError, match="shape-generic"):
            eng.set_split_precision(mode)
        assert eng.get_option(_lib.PD_OPT_DENOISER_SPLIT) == 0
    eng.set_split_precision(0)
    x, z = torch.randn(2, 20, 9).to(DEV), torch.randn(2, 20, cfg.z).to(DEV)
    a = eng.denoise(x, z, 10)
    for v in (0, 2, 1):
        eng.set_option(_lib.PD_OPT_DENOISER_FUSED_ATTN, v)
        assert eng.get_option(_lib.PD_OPT_DENOISER_FUSED_ATTN) == v
        assert torch.equal(eng.denoise(x, z, 10), a)
    # a default-shape engine keeps its options: split modes build, the fused-attention switch is read back
    d = _engine(seeded_diffuser.model, 52, 20)
    try:
        assert d.get_option(_lib.PD_OPT_DENOISER_SPLIT) == 2          # >= 1 024 token rows: the fp16-plane mode by default
        d.set_split_precision(1)
        assert d.get_option(_lib.PD_OPT_DENOISER_SPLIT) == 1
        d.set_split_precision(0)
        assert d.get_option(_lib.PD_OPT_DENOISER_SPLIT) == 0
    finally:
        d.close()


def test_pose_diffusion_model_with_non_default_transformer():
    """PoseDiffusionModel built from a Hydra-style MODEL node whose DENOISER.TRANSFORMER is d_model 256 / 8 heads (the shipped ViT,
    z 384): forward on 20 images samples and decodes to cameras."""
    import copy
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_synthetic_ckpt as mk
    from posediffusion_amd.compat import AttrDict, instantiate
    model_cfg = copy.deepcopy(mk.DEFAULT_MODEL_CFG)
    model_cfg["DENOISER"]["TRANSFORMER"].update(d_model=256, nhead=8, dim_feedforward=512, num_encoder_layers=4)
    synth._dropin()
    torch.manual_seed(0)
    model = instantiate(AttrDict(model_cfg), _recursive_=False).to(DEV).eval()
    assert model.diffuser.model._first.out_features == 256
    images = torch.rand(1, 20, 3, 224, 224, generator=torch.Generator().manual_seed(9)).to(DEV)
    torch.manual_seed(1)
    with torch.no_grad():
        out = model(image=images, training=False)
    cams = out["pred_cameras"]
    assert out["z"].shape == (1, 20, 384)
    for v in (cams.R, cams.T, cams.focal_length, out["pose_encoding"]):
        assert torch.isfinite(v).all()
    assert cams.R.shape[-2:] == (3, 3) and cams.R.numel() == 20 * 9
