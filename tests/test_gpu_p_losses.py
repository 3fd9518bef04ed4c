"""GPU (-m gpu): one timestep per sequence -- PoseEngine.denoise_t / p_losses (pd_denoise_step_t, pd_p_losses), the drop-in
Denoiser.forward(x, t[B], z), GaussianDiffusion.p_losses / forward and PoseDiffusionModel(training=True).

  * The reference's own p_losses outputs (tests/golden/p_losses.npz, tools/make_p_losses_golden.py) on a default engine, a
    PD_WEIGHTS_GENERIC engine and under objective pred_x0: model_out and x_t within TOL per column group; x_0_pred and the loss --
    amplified by sqrt_recipm1_alphas_cumprod[t], ~12 at t = 99 -- against the fp64 oracle within max(TOL, 4 x the fixture's own fp32
    distance from it) (the rule of tests/test_gpu_vit_tokens.py).
  * A t_seq whose entries are all equal is BITWISE the single-t launch, on the small path (1 023 rows), the large paths (1 024, 1 040,
    1 037 rows; every split mode) and the generic path.
  * Distinct timesteps against fp64 on the same shapes and modes, on the sequences around the 32 / 64 / 96-row tile boundaries; a
    sequence's result does not depend on the other sequences' timesteps.
  * Out-of-range timesteps are clamped on the device and reported by check_async().

TOL = 2e-5 is the teacher-forced denoiser bound of tests/test_gpu_denoiser_cfgs.py; every comparison is per column group (pose_err).

Measured on MI355X (this test writes profiles/p_losses_parity.txt): model_out within 9.7e-7
(default, pred_x0) / 2.0e-6 (generic) of the fixture, x_t bitwise the fixture's; x_0_pred 1.1e-6 (the fixture's own distance from fp64:
9.8e-7), 5.1e-6 under pred_x0 (4.9e-6); losses 1.0e-6 (l1) / 1.6e-6 (l2), the fixture's own figures.  denoise_t with distinct t against
fp64: 1.2e-6 - 1.8e-6 on every path and mode.
"""
import os

import pytest
import torch

from conftest import ROOT, load_golden, pose_err, pose_group_errs
from denoiser_cfgs import CONFIGS, build_dropin, fp64_copy, fp64_forward
from oracle import pd_oracle as O
from p_losses_cases import CASES, LOSS_TYPES, fp64_p_losses, inputs
from posediffusion_amd import synth
from posediffusion_amd.engine import PoseEngine
from posediffusion_amd.host import denoiser_state, get_engine
from posediffusion_amd.schedule import diffusion_buffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5
T = 100


def _engine(den, max_B, max_N, generic=False, objective="pred_noise"):
    return PoseEngine(denoiser_state(den), diffusion_buffers(), device=torch.device(DEV), max_B=max_B, max_N=max_N,
                      num_layers=len(den._trunk.layers), nhead=den._trunk.layers[0].self_attn.num_heads,
                      norm_first=den._trunk.layers[0].norm_first, pivot=den.pivot_cam_onehot, generic=generic, objective=objective)


# ------------------------------------------------------------------------------------------------ the reference's p_losses
@pytest.fixture(scope="module")
def sd64(oracle_weights):
    return O.cast_state_dict(oracle_weights, torch.float64)


@pytest.fixture(scope="module")
def fp64_cases(sd64):
    """Per case: the inputs and the fp64 model output at the fp64 x_t (objective-independent), computed once for the three engines."""
    tb = O.diffusion_tables(dtype=torch.float64)
    out = []
    for ci in range(len(CASES)):
        inp = inputs(ci)
        x_t = fp64_p_losses(torch.zeros_like(inp["x_start"]), inp["x_start"], inp["noise"], inp["t"], "pred_x0", tb)["x_t"]
        out.append((inp, O.denoiser_forward(sd64, x_t, inp["t"], inp["z"].double()), tb))
    return out


_PARITY = {}


def _write_parity():
    if {k[0] for k in _PARITY} != {"default", "generic", "pred_x0"}:           # the file holds a whole run of the three engines, never a part
        return
    try:
        with open(os.path.join(ROOT, "profiles", "p_losses_parity.txt"), "w") as fh:
            fh.write("PoseEngine.p_losses against tests/golden/p_losses.npz (model_out, x_t: bound 2e-5) and against the fp64 oracle\n"
                     "(x_0_pred, loss: bound max(2e-5, 4 x the fixture's own distance from fp64)); worst per-column-group relative error\n"
                     "over the four cases and both loss types.  variant / quantity: measured (bound; fixture's own distance)\n")
            for k in sorted(_PARITY):
                e, bound, own = _PARITY[k]
                fh.write(f"{k[0]:12s} {k[1]:10s} {e:.3e}  ({bound:.3e}; {own:.3e})\n")
    except OSError:
        pass


@pytest.mark.parametrize("variant", ["default", "generic", "pred_x0"])
def test_p_losses_vs_reference_fixture(variant, seeded_diffuser, fp64_cases):
    gold = load_golden("p_losses.npz")
    obj = "pred_x0" if variant == "pred_x0" else "pred_noise"
    eng = _engine(seeded_diffuser.model, 5, 64, generic=variant == "generic", objective=obj)
    try:
        for ci, c in enumerate(CASES):
            inp, mo64, tb = fp64_cases[ci]
            want = fp64_p_losses(mo64, inp["x_start"], inp["noise"], inp["t"], obj, tb)
            get = lambda k: torch.from_numpy(gold[f"{c.name}_{obj}_{k}"])          # noqa: E731
            for lt in LOSS_TYPES:
                out = eng.p_losses(inp["x_start"].to(DEV), inp["z"].to(DEV), inp["t"].to(DEV), inp["noise"].to(DEV), lt)
                eng.check_async()
                checks = [("model_out", out["model_out"], get("model_out"), None), ("x_t", out["x_t"], get("x_t"), None),
                          ("x_0_pred", out["x_0_pred"], want["x_0_pred"], get("x_0_pred")),
                          (f"loss_{lt}", out["loss"], want[f"loss_{lt}"], get(f"loss_{lt}"))]
                for name, got, ref, fixture in checks:
                    assert torch.isfinite(got).all()
                    own = 0.0 if fixture is None else pose_err(fixture, ref)
                    bound = max(TOL, 4.0 * own)
                    e = pose_err(got, ref, tag=f"p_losses/{variant}")
                    print(f"p_losses {variant} {c.name} {name}: {e:.3e} (bound {bound:.3e}, fixture's own distance {own:.3e})")
                    w = _PARITY.get((variant, name), (0.0, 0.0, 0.0))
                    if e >= w[0]:
                        _PARITY[(variant, name)] = (e, bound, own)
                    assert e < bound, (variant, c.name, name, pose_group_errs(got, ref), bound)
    finally:
        eng.close()
        _write_parity()


def test_p_losses_argument_errors(seeded_diffuser):
    eng = _engine(seeded_diffuser.model, 2, 4)
    try:
        x, z, t = torch.zeros(2, 4, 9, device=DEV), torch.zeros(2, 4, 384, device=DEV), torch.tensor([1, 2], device=DEV)
        with pytest.raises(ValueError, match="invalid loss type"):
            eng.p_losses(x, z, t, x, "huber")
        with pytest.raises(ValueError, match="one timestep per sequence"):
            eng.denoise_t(x, z, torch.tensor([1, 2, 3]))
        with pytest.raises(RuntimeError, match="invalid arguments"):
            eng.denoise_t(torch.zeros(3, 4, 9, device=DEV), torch.zeros(3, 4, 384, device=DEV), torch.tensor([1, 2, 3]))   # B > max_B
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ uniform / distinct t on every path
SMALL = [(33, 31)]                                  # 1 023 rows: the last small-path size
LARGE = [(16, 64), (52, 20), (17, 61)]              # 1 024 rows; 1 040 rows, sequences straddle rows 32 / 64 / 96; 1 037 rows, no multiple of 4
PATHS = [(s, None) for s in SMALL] + [(s, m) for s in LARGE for m in (2, 0, 1)]
_IDS = [f"b{s[0]}n{s[1]}" + ("" if m is None else f"_split{m}") for s, m in PATHS]


@pytest.fixture(scope="module")
def big_engine(seeded_diffuser):
    eng = _engine(seeded_diffuser.model, 52, 64)
    yield eng
    eng.close()


def _batch(B, N, zdim=384):
    g = torch.Generator().manual_seed(B * 1000 + N)
    x, z = torch.randn(B, N, 9, generator=g), torch.randn(B, N, zdim, generator=g)
    t = torch.randint(0, T, (B,), generator=g)          # a fixed draw with repeats (B > 1) ...
    t[1], t[B - 1] = 0, T - 1                           # ... that holds both ends of the schedule, on sequences that are compared
    kept = sorted({0, 1, B // 2, B - 1} | {r // N for r in (31, 32, 63, 64, 95, 96) if r < B * N})
    return x, z, t, kept


def _set_mode(eng, mode):
    if mode is not None:
        eng.set_split_precision(mode)


@pytest.mark.parametrize("shape,mode", PATHS, ids=_IDS)
def test_uniform_t_is_bitwise_the_single_t_launch(big_engine, shape, mode):
    B, N = shape
    x, z, _, _ = _batch(B, N)
    x, z = x.to(DEV), z.to(DEV)
    _set_mode(big_engine, mode)
    try:
        for t in (0, 50, 99):
            a = big_engine.denoise(x, z, t)
            b = big_engine.denoise_t(x, z, torch.full((B,), t, dtype=torch.long))
            assert torch.isfinite(a).all() and torch.equal(a, b), (shape, mode, t, (a - b).abs().max().item())
        big_engine.check_async()
    finally:
        _set_mode(big_engine, 2)


_FP64 = {}


def _fp64_kept(sd64, shape):
    if shape not in _FP64:
        x, z, t, kept = _batch(*shape)
        _FP64[shape] = O.denoiser_forward(sd64, x[kept].double(), t[kept], z[kept].double())
    return _FP64[shape]


@pytest.mark.parametrize("shape,mode", [p for p in PATHS if p[1] != 1], ids=[i for i, p in zip(_IDS, PATHS) if p[1] != 1])
def test_distinct_t_vs_fp64_and_independent_of_the_other_sequences(big_engine, sd64, shape, mode):
    """(mode 1, the bf16 planes, is narrower than fp32 by design and is covered by the bitwise test only)"""
    B, N = shape
    x, z, t, kept = _batch(B, N)
    assert len(set(t.tolist())) > 1 and 0 in t.tolist() and T - 1 in t.tolist()
    ref = _fp64_kept(sd64, shape)
    _set_mode(big_engine, mode)
    try:
        out = big_engine.denoise_t(x.to(DEV), z.to(DEV), t.to(DEV))
        e = pose_err(out[kept], ref, tag="denoise_t/fp64")
        print(f"denoise_t {shape} split {mode}: {e:.3e} on sequences {kept}")
        assert e < TOL, (shape, mode, pose_group_errs(out[kept], ref))
        t2 = t.clone()
        others = [b for b in range(B) if b not in kept]
        t2[others] = (t[others] + 37) % T
        assert not torch.equal(t2, t)
        out2 = big_engine.denoise_t(x.to(DEV), z.to(DEV), t2.to(DEV))
        assert torch.equal(out2[kept], out[kept])
        assert not torch.equal(out2[others], out[others])
        big_engine.check_async()
    finally:
        _set_mode(big_engine, 2)


@pytest.mark.parametrize("shape", [(5, 13), (52, 20)], ids=["b5n13", "b52n20"])
def test_generic_path_uniform_bitwise_and_distinct_vs_fp64(shape):
    cfg = CONFIGS[4]                                    # d 96, 3 heads, post-norm, no pivot: the shape-generic kernels
    assert not cfg.norm_first and not cfg.pivot
    den = build_dropin(cfg, seed=21)
    B, N = shape
    x, z, t, kept = _batch(B, N, cfg.z)
    eng = _engine(den, B, N)
    try:
        for tt in (0, 50, 99):
            assert torch.equal(eng.denoise(x.to(DEV), z.to(DEV), tt), eng.denoise_t(x.to(DEV), z.to(DEV), torch.full((B,), tt)))
        out = eng.denoise_t(x.to(DEV), z.to(DEV), t)
        ref = fp64_forward(fp64_copy(den), x[kept], t[kept], z[kept])
        e = pose_err(out[kept], ref, tag="denoise_t/generic")
        assert e < TOL, (shape, pose_group_errs(out[kept], ref))
        t2 = t.clone()
        others = [b for b in range(B) if b not in kept]
        if others:
            t2[others] = (t[others] + 37) % T
            assert torch.equal(eng.denoise_t(x.to(DEV), z.to(DEV), t2)[kept], out[kept])
        eng.check_async()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ the drop-in modules
@pytest.fixture(scope="module")
def gpu_diffuser():
    diff = synth.make_diffuser(seed=0)
    synth.randomize_norm_and_bias_(diff.model)
    return diff.to(DEV)


def test_dropin_denoiser_forward_with_per_sequence_t(gpu_diffuser, sd64):
    B, N = 6, 7
    x, z, t, _ = _batch(B, N)
    den = gpu_diffuser.model
    out = den(x.to(DEV), t.to(DEV), z.to(DEV))
    ref = O.denoiser_forward(sd64, x.double(), t, z.double())
    assert pose_err(out, ref, tag="denoise_t/dropin") < TOL
    assert torch.equal(out, get_engine(den, None, B, N).denoise_t(x.to(DEV), z.to(DEV), t))
    same = den(x.to(DEV), torch.full((B,), 7), z.to(DEV))                       # the uniform case stays on the single-t launch
    assert torch.equal(same, get_engine(den, None, B, N).denoise(x.to(DEV), z.to(DEV), 7))
    with pytest.raises(ValueError, match="timesteps must lie in"):
        den(x.to(DEV), torch.tensor([0, 1, 2, 3, 4, T]), z.to(DEV))


def test_out_of_range_t_is_clamped_and_reported(gpu_diffuser):
    B, N = 2, 5
    x, z, _, _ = _batch(B, N)
    x, z = x.to(DEV), z.to(DEV)
    eng = get_engine(gpu_diffuser.model, gpu_diffuser, B, N)
    eng.check_async()
    bad = torch.tensor([-1, T], device=DEV)
    out = eng.denoise_t(x, z, bad)
    assert torch.isfinite(out).all()
    with pytest.raises(RuntimeError, match="timestep outside"):
        eng.check_async()
    eng.check_async()                                                          # the word was cleared
    ok = eng.denoise_t(x, z, torch.tensor([0, T - 1], device=DEV))
    eng.check_async()
    assert torch.equal(out, ok)                                                # clamped to the ends of the schedule
    res = eng.p_losses(x, z, bad, torch.ones_like(x), "l2")
    assert all(torch.isfinite(v).all() for v in res.values())
    with pytest.raises(RuntimeError, match="timestep outside"):
        eng.check_async()
    good = eng.p_losses(x, z, torch.tensor([0, T - 1], device=DEV), torch.ones_like(x), "l2")
    eng.check_async()
    assert all(torch.equal(res[k], good[k]) for k in res)


@pytest.mark.parametrize("objective,loss_type", [("pred_noise", "l1"), ("pred_noise", "l2"), ("pred_x0", "l1"), ("pred_x0", "l2")])
def test_dropin_p_losses_and_forward(gpu_diffuser, sd64, objective, loss_type):
    """GaussianDiffusion.p_losses returns the reference's dict; its entries follow from the engine's model output by the fp64 formulas."""
    B, N = 3, 5
    inp = inputs(1)
    old = gpu_diffuser.objective, gpu_diffuser.loss_type
    gpu_diffuser.objective, gpu_diffuser.loss_type = objective, loss_type
    try:
        r = gpu_diffuser.p_losses(inp["x_start"].to(DEV), inp["t"].to(DEV), z=inp["z"].to(DEV), noise=inp["noise"].to(DEV))
        assert sorted(r) == ["loss", "noise", "t", "x_0_pred", "x_t"]
        assert torch.equal(r["t"].cpu(), inp["t"]) and torch.equal(r["noise"].cpu(), inp["noise"])
        assert not any(v.requires_grad for v in r.values())
        tb = O.diffusion_tables(dtype=torch.float64)
        x_t = fp64_p_losses(torch.zeros(B, N, 9), inp["x_start"], inp["noise"], inp["t"], "pred_x0", tb)["x_t"]
        want = fp64_p_losses(O.denoiser_forward(sd64, x_t, inp["t"], inp["z"].double()), inp["x_start"], inp["noise"], inp["t"], objective, tb)
        assert pose_err(r["x_t"], want["x_t"]) < TOL
        # x_0_pred / loss: the reference's own fp32 results sit this far from fp64 on this case (tests/golden/p_losses.npz, case b3n5)
        gold = load_golden("p_losses.npz")
        for k, w in (("x_0_pred", want["x_0_pred"]), ("loss", want[f"loss_{loss_type}"])):
            own = pose_err(gold[f"b3n5_{objective}_{k if k != 'loss' else 'loss_' + loss_type}"], w)
            assert pose_err(r[k], w) < max(TOL, 4.0 * own), (k, pose_group_errs(r[k], w), own)
        torch.manual_seed(5)
        f = gpu_diffuser(inp["x_start"].to(DEV), z=inp["z"].to(DEV))
        torch.manual_seed(5)
        t = torch.randint(0, T, (B,), device=DEV).long()                       # gaussian_diffuser.py:331: the first draw of forward
        assert torch.equal(f["t"], t) and f["t"].device.type == "cuda"
        again = gpu_diffuser.p_losses(inp["x_start"].to(DEV), f["t"], z=inp["z"].to(DEV), noise=f["noise"])
        assert all(torch.equal(f[k], again[k]) for k in f)
        with pytest.raises(NotImplementedError):
            gpu_diffuser(inp["x_start"].to(DEV))
    finally:
        gpu_diffuser.objective, gpu_diffuser.loss_type = old


def test_pose_diffusion_model_training_branch():
    """PoseDiffusionModel(image=None, gt_cameras=cams, training=True, z=z) (pose_diffusion_model.py:111-126)."""
    import numpy as np
    from posediffusion_amd.compat import AttrDict, PerspectiveCameras
    models = synth._dropin()
    from util.camera_transform import camera_to_pose_encoding
    cfg = {"pose_encoding_type": "absT_quaR_logFL",
           "IMAGE_FEATURE_EXTRACTOR": AttrDict({"_target_": "models.MultiScaleImageFeatureExtractor", "freeze": False}),
           "DENOISER": AttrDict({"_target_": "models.Denoiser", "TRANSFORMER": AttrDict(synth.TRANSFORMER_CFG)}),
           "DIFFUSER": AttrDict({"_target_": "models.GaussianDiffusion", "beta_schedule": "custom"})}
    torch.manual_seed(0)
    model = models.PoseDiffusionModel(**cfg).to(DEV).eval()
    B, N = 2, 5

    def cameras(n_seq, seed):
        enc = torch.from_numpy(np.concatenate([synth.make_cameras(N, seed=seed + b) for b in range(n_seq)])).float()
        c = O.pose_encoding_to_camera(enc)
        return enc, PerspectiveCameras(focal_length=c["focal_length"].to(DEV), R=c["R"].to(DEV), T=c["T"].to(DEV), device=torch.device(DEV))

    enc, cams = cameras(B, 300)
    z = synth.make_z(B, N).to(DEV)
    torch.manual_seed(1)
    out = model(image=None, gt_cameras=cams, training=True, z=z)
    assert sorted(out) == ["loss", "noise", "pred_cameras", "t", "x_0_pred", "x_t"]
    assert out["loss"].shape == (B, N, 9) and out["t"].shape == (B,)
    eng = get_engine(model.diffuser.model, model.diffuser, B, N)
    got = camera_to_pose_encoding(cams, engine=eng)
    known = enc.clone()
    known[:, 3:7] = enc[:, 3:7] / enc[:, 3:7].norm(dim=-1, keepdim=True)        # the encoding of a camera holds the UNIT quaternion
    assert pose_err(got, known) < 1e-5 and torch.equal(got[:, :3].cpu(), enc[:, :3])
    r = model.diffuser.p_losses(got.reshape(B, N, 9), out["t"], z=z, noise=out["noise"])
    for k in ("x_t", "loss", "x_0_pred"):
        assert torch.equal(out[k], r[k]), k
    R, Tr, F = eng.pose_to_camera(out["x_0_pred"])
    pc = out["pred_cameras"]
    assert torch.equal(pc.R, R) and torch.equal(pc.T, Tr) and torch.equal(pc.focal_length, F)
    _, cams2 = cameras(2 * B, 400)
    out2 = model(image=None, gt_cameras=cams2, training=True, z=z, batch_repeat=2)
    assert out2["loss"].shape == (2 * B, N, 9) and out2["t"].shape == (2 * B,) and out2["pred_cameras"].R.shape == (2 * B * N, 3, 3)
    with pytest.raises(NotImplementedError, match="ground-truth cameras"):
        model(image=None, training=True, z=z)
