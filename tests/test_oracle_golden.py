"""CPU: the oracle restatement against (a) the committed golden vectors produced by the reference's own
files and (b) the reference's outputs on small cases, recorded by oracle/make_golden.py (live_reference.npz).  Tolerances are fp32 rounding
class (the oracle runs 8 threads / different BLAS blocking than the single-threaded fixture run)."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import pd_oracle as O
from posediffusion_amd import synth

FLAGS = {"all": (True, True, True), "fl": (False, False, True), "r": (True, False, False), "t": (False, True, False)}


def test_schedule_tables_bit_exact(golden):
    t = O.diffusion_tables()
    for n in O.TABLE_NAMES:
        assert np.array_equal(t[n].numpy(), golden["tables"][n]), n
    # SURVEY.md section 8c spot values
    assert abs(t["sqrt_recip_alphas_cumprod"][99].item() - 13.340734) < 1e-5
    assert abs(t["posterior_log_variance_clipped"][0].item() + 46.0517) < 1e-3
    assert abs(t["posterior_mean_coef2"][99].item() - 0.94808769) < 1e-7


@pytest.mark.parametrize("case", ["b2n20", "b1n7", "b3n33"])
def test_denoiser_forward_golden(golden, oracle_weights, case):
    d = golden["denoiser"]
    x, z = torch.from_numpy(d[f"{case}_x"]), torch.from_numpy(d[f"{case}_z"])
    for t in (99, 50, 0):
        out = O.denoiser_forward(oracle_weights, x, torch.full((x.shape[0],), t, dtype=torch.long), z)
        assert rel_err(out, d[f"{case}_eps_t{t}"]) < 5e-6


def test_p_sample_golden(golden, oracle_weights):
    d = golden["denoiser"]
    tables = O.diffusion_tables()
    x, z = torch.from_numpy(d["b2n20_x"]), torch.from_numpy(d["b2n20_z"])
    for t in (99, 50, 10, 9, 0):
        noise = torch.from_numpy(d[f"ps_noise_t{t}"])
        pred, x0 = O.p_sample(oracle_weights, tables, x, t, z, noise if t > 0 else None)
        assert rel_err(pred, d[f"ps_pred_t{t}"]) < 5e-6
        assert rel_err(x0, d[f"ps_x0_t{t}"]) < 5e-6


def test_objective_pred_x0_golden(golden, oracle_weights, seeded_diffuser):
    """GaussianDiffusion(objective="pred_x0") (models/gaussian_diffuser.py:225-227): the oracle's p_sample against the reference's
    at five steps and teacher-forced along the reference's whole trajectory; the drop-in module's schedule helpers
    (predict_noise_from_start / predict_start_from_noise / q_posterior, :190-209) against the reference's model_predictions pair."""
    d = golden["pred_x0"]
    tables = O.diffusion_tables()
    x, z = torch.from_numpy(d["x"]), torch.from_numpy(d["z"])
    for t in (99, 50, 10, 1, 0):
        pred, x0 = O.p_sample(oracle_weights, tables, x, t, z, torch.from_numpy(d[f"ps_noise_t{t}"]) if t > 0 else None, objective="pred_x0")
        assert rel_err(pred, d[f"ps_pred_t{t}"]) < 5e-6 and rel_err(x0, d[f"ps_x0_t{t}"]) < 5e-6
    proc, noise, zt = torch.from_numpy(d["traj_process"]), torch.from_numpy(d["traj_noise"]), torch.from_numpy(d["traj_z"])
    for step in list(range(0, 100, 10)) + [99]:
        t = 99 - step
        nxt, _ = O.p_sample(oracle_weights, tables, proc[step], t, zt, noise[step + 1] if t > 0 else None, objective="pred_x0")
        assert rel_err(nxt, proc[step + 1]) < 5e-6
    # iterating an untrained network as its own x_start is chaotic over the last ~25 steps (fp32 vs fp64: 5e-6 at step 70, 0.15 at
    # step 100): the free-running comparison of tests/test_gpu_parity_r3.py stops at step 70
    dev = np.abs(d["traj_process"].astype(np.float64) - d["traj_process64"]).max(axis=(1, 2, 3))
    assert dev[70] < 2e-5 and dev[100] > 1e-3
    # the drop-in module's helpers, on the CPU (they are plain buffer arithmetic; the sampler fuses them into pd_tail_kernel)
    GaussianDiffusion = synth._dropin().GaussianDiffusion
    diff = GaussianDiffusion(beta_schedule="custom", objective="pred_x0")
    tt = torch.full((x.shape[0],), 50, dtype=torch.long)
    x0 = torch.from_numpy(d["mp_x0_t50"])
    pn = diff.predict_noise_from_start(x, tt, x0)
    assert rel_err(pn, d["mp_noise_t50"]) < 1e-6
    assert rel_err(diff.predict_start_from_noise(x, tt, pn), x0) < 1e-5
    assert rel_err(diff.predict_start_from_noise(x, 50, pn), x0) < 1e-5                     # an int t is accepted as well
    mean, var, logvar = diff.q_posterior(x0, x, tt)
    assert rel_err(mean, d["ps_pred_t50"] - np.exp(0.5 * float(logvar[0, 0, 0])) * d["ps_noise_t50"]) < 1e-5
    assert mean.shape == x.shape and var.shape == (2, 1, 1) and diff.loss_fn is torch.nn.functional.l1_loss
    xs = diff.q_sample(x0, tt, noise=torch.zeros_like(x0))
    assert rel_err(xs, float(diff.sqrt_alphas_cumprod[50]) * x0) < 1e-6


def _pm(g, prefix=""):
    return O.prepare_matches(g[prefix + "kp1"], g[prefix + "kp2"], g[prefix + "i12"], tuple(int(v) for v in g["img_shape"]))


@pytest.mark.parametrize("fname", list(FLAGS))
@pytest.mark.parametrize("smax", [10, 0.3])
def test_sampson_value_and_gradient_golden(golden, fname, smax):
    g = golden["ggs"]
    pm = _pm(g)
    x = torch.from_numpy(g["x0"]).clone().requires_grad_(True)
    v, pr = O.compute_sampson_distance(x, pm, *FLAGS[fname], sampson_max=smax)
    (grad,) = torch.autograd.grad(v.mean(), x)
    tag = f"sam_{fname}_max{smax}"
    assert len(v) == int(g[tag + "_nvalid"])
    # fp32 means over the valid matches: the summation order depends on the host (vector width, thread partition); the fixture
    # was written on another CPU than the GPU box's (3.5e-6 apart there at sampson_max = 0.3, where few matches survive)
    assert abs(v.mean().item() - float(g[tag + "_loss"])) < 2e-5 * abs(float(g[tag + "_loss"]))
    assert abs(pr.item() - float(g[tag + "_print"])) < 2e-5 * abs(float(g[tag + "_print"]))
    assert rel_err(grad, g[tag + "_grad"]) < 1e-4           # host dependent likewise (2e-6 here, 4e-5 on the GPU box's CPU)


def test_analytic_backward_matches_autograd_fp64(golden):
    """The hand-derived backward the HIP kernel implements == torch autograd (fp64), all flag sets."""
    g = golden["ggs"]
    pm = _pm(g)
    kp1 = g["kp1"].astype(np.float32).astype(np.float64)      # the .float() cast of geometry_guided_sampling.py:167
    kp2 = g["kp2"].astype(np.float32).astype(np.float64)
    pm32 = dict(pm, kp1_homo=torch.from_numpy(np.concatenate([kp1, np.ones((len(kp1), 1))], 1)),
                kp2_homo=torch.from_numpy(np.concatenate([kp2, np.ones((len(kp2), 1))], 1)))
    for xk in ("x0", "clamp_x"):
        for flags in FLAGS.values():
            x = torch.from_numpy(g[xk]).double().clone().requires_grad_(True)
            v, pr = O.compute_sampson_distance(x, pm32, *flags)
            (grad,) = torch.autograd.grad(v.mean(), x)
            loss, cnt, ga, pa = O.sampson_loss_grad_analytic(g[xk][0], kp1, kp2, g["i12"][:, 0], g["i12"][:, 1], 224, 224, *flags)
            assert cnt == len(v)
            assert abs(loss - v.mean().item()) < 1e-12 * abs(loss)
            assert abs(pa - pr.item()) < 1e-12 * abs(pa)
            assert np.abs(ga - grad[0].numpy()).max() < 1e-10 * np.abs(grad.numpy()).max()


def test_focal_clamp_edges_golden(golden):
    g = golden["ggs"]
    x = torch.from_numpy(g["clamp_x"]).clone().requires_grad_(True)
    v, _ = O.compute_sampson_distance(x, _pm(g))
    (grad,) = torch.autograd.grad(v.mean(), x)
    assert len(v) == int(g["clamp_nvalid"])
    assert rel_err(grad, g["clamp_grad"]) < 2e-5
    assert (grad[0, 0, 7:9] == 0).all() and (grad[0, 1, 7:9] == 0).all()      # clamped frames get no focal gradient


@pytest.mark.parametrize("tag", ["default", "a", "b"])
def test_pose_decode_parameters_golden(golden, tag):
    """The oracle's pose_encoding_to_camera against the reference's (executed in place by oracle/make_golden.py decode_args) at the default
    and two non-default (log_focal_length_bias, min_focal_length, max_focal_length) -- util/camera_transform.py:64-70, :89-97."""
    g = golden["decode_args"]
    bias, fmin, fmax = (float(v) for v in g[f"{tag}_args"])
    d = O.pose_encoding_to_camera(torch.from_numpy(g["enc"]), bias, fmin, fmax)
    assert np.array_equal(d["T"].numpy(), g[f"{tag}_T"])
    assert rel_err(d["R"], g[f"{tag}_R"]) < 1e-6 and rel_err(d["focal_length"], g[f"{tag}_focal"]) < 1e-6
    f = g[f"{tag}_focal"]
    assert (f == np.float32(fmin)).any() and (f == np.float32(fmax)).any() and ((f > fmin) & (f < fmax)).any(), "the fixture straddles both clamps"


@pytest.mark.parametrize("fname", ["all", "fl", "r"])
@pytest.mark.parametrize("k", [1, 5, 20])
def test_ggs_optimize_iterations_golden(golden, fname, k):
    g = golden["ggs"]
    xo, _, steps = O.ggs_optimize(torch.from_numpy(g["x0"]).clone(), _pm(g), *FLAGS[fname], iter_num=k)
    assert steps == (2 * k if fname == "all" else k)
    # iterated results drift with thread count / summation order (the reference itself: 3e-4 .. 5e-4 over
    # 700 iterations, SURVEY.md headline fact 4); 20 iterations stay within 1e-5
    assert rel_err(xo, g[f"opt_{fname}_k{k}"]) < 1e-5


def test_geometry_guided_sampling_golden(golden):
    g = golden["ggs"]
    md = {"kp1": g["kp1"], "kp2": g["kp2"], "i12": g["i12"], "img_shape": tuple(int(v) for v in g["img_shape"])}
    from posediffusion_amd.synth import GGS_CFG
    xo = O.geometry_guided_sampling(torch.from_numpy(g["x0"]).clone(), 3, md, dict(GGS_CFG, iter_num=10))
    assert rel_err(xo, g["guide_k10"]) < 2e-5


@pytest.mark.parametrize("setting", ["default", "never_clipped", "crossing"])
def test_ggs_on_a_non_square_image_and_outside_the_clipped_regime_golden(golden, setting):
    """The oracle in fp32 against tests/golden/ggs_inputs.npz (the reference executed in place on a 192 x 320 scene at three settings of
    (alpha, learning_rate): oracle/make_golden.py ggs_inputs), under the bounds of the square fixture's tests above.  The scene and the
    settings are the ones tests/ggs_input_cases.py hands the GPU tests."""
    import ggs_input_cases as Cs
    g = golden["ggs_inputs"]
    md, _, x0c = Cs.scene(*Cs.FIXTURE_SCENE)
    assert tuple(int(v) for v in g["img_shape"]) == (6, 3, 192, 320) == tuple(md["img_shape"])
    assert np.array_equal(g["kp1"], md["kp1"]) and np.array_equal(g["kp2"], md["kp2"]) and np.array_equal(g["i12"], md["i12"])
    assert np.array_equal(g["x0"], x0c.numpy())
    cfg = Cs.cfg_of(setting, Cs.FIXTURE_SCENE)
    assert [cfg["alpha"], cfg["learning_rate"]] == g[f"{setting}_alpha_lr"].tolist()
    pm, x0 = _pm(g), torch.from_numpy(g["x0"])
    for fname, flags in FLAGS.items():
        if setting == "default":                                 # (the Sampson values do not depend on the optimiser's settings)
            x = x0.clone().requires_grad_(True)
            v, pr = O.compute_sampson_distance(x, pm, *flags)
            (grad,) = torch.autograd.grad(v.mean(), x)
            tag = f"sam_{fname}"
            assert len(v) == int(g[tag + "_nvalid"])
            assert rel_err(v, g[tag + "_values"]) < 2e-5
            assert abs(v.mean().item() - float(g[tag + "_loss"])) < 2e-5 * abs(float(g[tag + "_loss"]))
            assert abs(pr.item() - float(g[tag + "_print"])) < 2e-5 * abs(float(g[tag + "_print"]))
            assert rel_err(grad, g[tag + "_grad"]) < 1e-4
        xo, _, steps = O.ggs_optimize(x0.clone(), pm, *flags, **dict(cfg, iter_num=3))
        assert steps == (6 if fname == "all" else 3)
        assert rel_err(xo, g[f"{setting}_opt_{fname}_k3"]) < 1e-5
    md_g = {"kp1": g["kp1"], "kp2": g["kp2"], "i12": g["i12"], "img_shape": tuple(int(v) for v in g["img_shape"])}
    assert rel_err(O.geometry_guided_sampling(x0.clone(), 3, md_g, dict(cfg, iter_num=2)), g[f"{setting}_guide_k2"]) < 2e-5
    # the settings differ where they should: the stored results are not one result three times
    if setting != "default":
        assert rel_err(g[f"{setting}_opt_all_k3"], g["default_opt_all_k3"]) > 1e-4


def test_early_exit_golden(golden):
    g = golden["ggs"]
    md = {"kp1": g["bad_kp1"], "kp2": g["bad_kp2"], "i12": g["bad_i12"], "img_shape": tuple(int(v) for v in g["img_shape"])}
    from posediffusion_amd.synth import GGS_CFG
    stats = []
    xo = O.geometry_guided_sampling(torch.from_numpy(g["x0"]).clone(), 3, md, dict(GGS_CFG, iter_num=10, sampson_max=0.01), stats)
    assert int(g["bad_dropped"]) == 5 and int(g["bad_nvalid_max0.01"]) < 10 * 8
    assert np.array_equal(xo.numpy(), g["bad_out"]) and np.array_equal(xo.numpy(), g["x0"])   # no step was taken


def test_trajectory_golden(golden, oracle_weights):
    """Teacher-forced: every 10th step of the reference's 100-step trajectory, fed the reference state."""
    tr = golden["trajectory"]
    tables = O.diffusion_tables()
    z = torch.from_numpy(tr["z"])
    proc, noise = torch.from_numpy(tr["process"]), torch.from_numpy(tr["noise"])
    for step in list(range(0, 100, 10)) + [99]:
        t = 99 - step
        nxt, _ = O.p_sample(oracle_weights, tables, proc[step], t, z, noise[step + 1] if t > 0 else None)
        assert rel_err(nxt, proc[step + 1]) < 5e-6
    # the reference-fp32 trajectory's own deviation from the fp64 oracle (context for the free-running metric)
    dev = rel_err(tr["process"][-1], tr["process64"][-1])
    assert dev < 2e-2


def test_noise_replay_matches_reference_order(golden):
    tr = golden["trajectory"]
    init, noises = O.draw_reference_noise((1, 20, 9), torch.Generator().manual_seed(0))
    assert np.array_equal(init.numpy(), tr["noise"][0])
    assert np.array_equal(noises[99].numpy(), tr["noise"][1]) and noises[0] is None


def test_oracle_against_live_reference(golden, oracle_weights):
    """The oracle against the reference executed in place on two small cases -- Denoiser.forward and a whole geometry_guided_sampling --
    whose inputs and outputs oracle/make_golden.py (`live_reference`) recorded in tests/golden/live_reference.npz."""
    g = golden["live_reference"]
    np.testing.assert_allclose(g["den_weight_checksum"], golden["denoiser"]["weight_checksum"], rtol=1e-9)
    x, z, tt = (torch.from_numpy(g[k]) for k in ("den_x", "den_z", "den_t"))
    assert rel_err(O.denoiser_forward(oracle_weights, x, tt, z), torch.from_numpy(g["den_eps"])) < 5e-6
    md = {"kp1": g["ggs_kp1"], "kp2": g["ggs_kp2"], "i12": g["ggs_i12"], "img_shape": tuple(int(v) for v in g["ggs_img_shape"])}
    cfg = dict(synth.GGS_CFG, iter_num=int(g["ggs_iter_num"]))
    x0 = torch.from_numpy(g["ggs_x0"])
    assert rel_err(O.geometry_guided_sampling(x0.clone(), int(g["ggs_t"]), md, cfg), torch.from_numpy(g["ggs_out"])) < 2e-5


# ---------------------------------------------------------------------------------------------- third-party helpers
# pytorch3d is neither under /root/reference nor installed, so its five helpers are restated in the oracle (parity
# against pytorch3d's source is unpinned).  These checks pin the restatements against INDEPENDENT
# definitions: scipy's rotation class, the cross product, and the documented PyTorch3D NDC projection convention.
def test_quaternion_to_matrix_against_scipy():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(0)
    q = rng.normal(size=(64, 4)) * rng.uniform(0.2, 5.0, size=(64, 1))            # real-first, NOT normalised
    ours = O.quaternion_to_matrix(torch.from_numpy(q)).numpy()
    ref = Rotation.from_quat(q[:, [1, 2, 3, 0]]).as_matrix()                       # scipy: scalar-last, normalises
    assert np.abs(ours - ref).max() < 1e-12
    assert np.abs(ours @ ours.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12      # the 2/|q|^2 scaling keeps R orthonormal


def test_hat_is_the_cross_product_matrix():
    rng = np.random.default_rng(1)
    v, w = rng.normal(size=(32, 3)), rng.normal(size=(32, 3))
    hv = O.hat(torch.from_numpy(v)).numpy()
    assert np.abs(np.einsum("bij,bj->bi", hv, w) - np.cross(v, w)).max() < 1e-14


def test_opencv_conversion_reproduces_the_ndc_projection():
    """PyTorch3D convention (documented): X_cam = X_world R + T (row vectors), x_ndc = f X/Z, +x left / +y up, so
    pixel u = W/2 - x_ndc s, v = H/2 - y_ndc s with s = min(H, W)/2.  The restated opencv_from_cameras_projection
    must give the same pixels through K (R_cv X + t_cv)."""
    rng = np.random.default_rng(2)
    n, H, W = 16, 224, 336
    q = rng.normal(size=(n, 4))
    R = O.quaternion_to_matrix(torch.from_numpy(q))
    T = torch.from_numpy(rng.normal(size=(n, 3)) * 0.3 + np.array([0.0, 0.0, 6.0]))
    f = torch.from_numpy(rng.uniform(1.0, 4.0, size=(n, 2)))
    X = torch.from_numpy(rng.normal(size=(n, 50, 3)))
    Xc = X @ R + T[:, None, :]
    s = min(H, W) / 2.0
    u = W / 2.0 - f[:, None, 0] * Xc[..., 0] / Xc[..., 2] * s
    v = H / 2.0 - f[:, None, 1] * Xc[..., 1] / Xc[..., 2] * s
    Rcv, tcv, K = O.opencv_from_cameras_projection(R, T, f, H, W)
    P = (K[:, None] @ ((Rcv[:, None] @ X[..., None]) + tcv[:, None, :, None]))[..., 0]
    assert (P[..., 2] > 0).all()
    assert torch.abs(P[..., 0] / P[..., 2] - u).max() < 1e-9 and torch.abs(P[..., 1] / P[..., 2] - v).max() < 1e-9


def test_harmonic_embedding_layout():
    """HarmonicEmbedding(n_harmonic_functions=10, append_input=True): [sin(x f) | cos(x f) | x], f = 2^k, dim-major."""
    x = torch.tensor([[0.3, -1.7, 2.0]], dtype=torch.float64)
    e = O.harmonic_embedding(x, 10)
    assert e.shape == (1, 3 * 10 * 2 + 3)
    fr = 2.0 ** np.arange(10)
    arg = (x.numpy()[0][:, None] * fr[None, :]).reshape(-1)
    assert np.abs(e[0, :30].numpy() - np.sin(arg)).max() < 1e-12
    # 0.7.x computes cos as sin(. + pi/2) with pi/2 held in float32 (4.4e-8 off): the restatement keeps that
    assert np.abs(e[0, 30:60].numpy() - np.cos(arg)).max() < 1e-7
    assert torch.equal(e[0, 60:], x[0])


# ---------------------------------------------------------------------------------------------- N3: evaluation metrics
def test_metrics_oracle_against_reference_fixture(golden):
    g = golden["metrics"]
    r, t = O.camera_to_rel_deg(torch.from_numpy(g["R_pred"]), torch.from_numpy(g["T_pred"]), torch.from_numpy(g["R_gt"]),
                               torch.from_numpy(g["T_gt"]), int(g["B"]))
    assert np.abs(r.numpy() - g["rel_r_deg"]).max() < 1e-5 and np.abs(t.numpy() - g["rel_t_deg"]).max() < 1e-5
    assert abs(O.calculate_auc_np(g["rel_r_deg"], g["rel_t_deg"]) - float(g["auc30"])) < 1e-12
    assert np.abs(O.compute_ARE(g["R_pred"], g["R_gt"]) - g["are_deg"]).max() < 1e-5


def test_metrics_oracle_against_reference_edge_fixture(golden):
    """O.compute_ARE / O.camera_to_rel_deg / O.calculate_auc_np on the edges recorded from the reference (oracle/make_golden.py
    make_metrics_edges): the fold of the ARE at 90 degrees, both extrapolated ends of the rotation angle, zero / parallel / orthogonal
    relative translations and the 1e6 default, every bin edge and threshold of the AUC, NaN and inf errors."""
    g = golden["metrics_edges"]
    are = O.compute_ARE(g["are_Ra"], g["are_Rb"])
    assert np.isnan(g["are_deg"]).tolist() == [False] * 20 + [True, False, True] and g["are_deg"][21] == 0.0      # NaN entry, inf trace, 0 * inf
    assert np.array_equal(np.isnan(are), np.isnan(g["are_deg"])) and np.nanmax(np.abs(are - g["are_deg"])) < 1e-5, (are, g["are_deg"])
    assert np.nanmax(g["are_deg"]) <= 90.0 and abs(g["are_deg"][7] - 60.0) < 1e-3    # 120 degrees reads 60
    default = np.float32(1e6) * np.float32(180.0 / np.pi)
    from metrics_checks import fixture_rel_case
    for name in g["rel_cases"]:
        c = fixture_rel_case(g, name)
        r, t = O.camera_to_rel_deg(*(torch.from_numpy(np.ascontiguousarray(c[k])) for k in ("Rp", "Tp", "Rg", "Tg")), c["B"])
        r, t, rr, tr = r.numpy(), t.numpy(), c["r"], c["t"]
        assert np.array_equal(np.isnan(r), np.isnan(rr)) and np.array_equal(np.isnan(t), np.isnan(tr)), name
        big = tr > 1e5                                                                 # the 1e6 rad default: by equality
        assert np.array_equal(t[big], tr[big]) and np.all(np.abs(tr[big] / default - 1) < 1e-6), name
        ok = ~np.isnan(rr)
        assert np.abs(r[ok] - rr[ok]).max() < 1e-5, name
        ok = ~np.isnan(tr) & ~big
        assert np.abs(t[ok] - tr[ok]).max() < 1e-5, name
    assert (g["trans_t"] > 1e5).sum() == 3 and np.isnan(g["trans_r"]).tolist() == [False] * 9 + [True, False, True] and (g["trans_t"] == 90.0).sum() >= 4
    for m, auc in zip(g["auc_thresholds"], g["auc"]):
        assert abs(O.calculate_auc_np(g["auc_r"], g["auc_t"], int(m)) - float(auc)) < 1e-12, m
        assert abs(O.calculate_auc_np(g["auc_r"].astype(np.float64), g["auc_t"].astype(np.float64), int(m)) - float(auc)) < 1e-12, m


def test_camera_alignment_recovers_a_similarity_exactly():
    """The restated pytorch3d alignment (unpinned against pytorch3d's source) must at least undo any similarity of the
    world: X' = s X R_A + T_A maps cameras (R, T) to (R_A^T R, s T - T_A R_A^T R)."""
    torch.manual_seed(3)
    n = 9
    R = O.quaternion_to_matrix(torch.randn(n, 4, dtype=torch.float64))
    T = torch.randn(n, 3, dtype=torch.float64)
    RA = O.quaternion_to_matrix(torch.randn(1, 4, dtype=torch.float64))[0]
    TA, s = torch.randn(3, dtype=torch.float64), 2.3
    Rt = RA.T[None] @ R
    Tt = s * T - (TA[None, None] @ Rt)[:, 0]
    Ral, Tal, (ra, ta, ss) = O.corresponding_cameras_alignment(R, T, Rt, Tt)
    assert (Ral - Rt).abs().max() < 1e-12 and (Tal - Tt).abs().max() < 1e-12 and abs(float(ss) - s) < 1e-12


# ---------------------------------------------------------------------------------------------- N1: image features
def test_multiscale_wrapper_against_live_reference(golden):
    """oracle/vit_oracle.multiscale_features (normalise, rescale by 1, 1/2, 1/3, average) against the reference's own
    models/image_feature_extractor.py executed in place around the same (restated) ViT, in fp64 (recorded by oracle/make_golden.py
    `live_reference`; fp64 so that the stored features do not depend on the host's BLAS and thread count)."""
    from oracle import vit_oracle as VO
    ref = torch.from_numpy(golden["live_reference"]["vit_features64"])
    net = VO.make_vit(seed=3, dtype=torch.float64)
    x = torch.rand(2, 3, 224, 224, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    with torch.no_grad():
        ours = VO.multiscale_features(net, x, (1, 1 / 2, 1 / 3))
    assert tuple(ref.shape) == (2, 384) and ours.dtype == torch.float64
    assert rel_err(ours, ref) < 1e-12


def test_vit_oracle_loads_dino_state_dict_names():
    from oracle import vit_oracle as VO
    keys = set(VO.make_vit(0).state_dict())
    for k in ("cls_token", "pos_embed", "patch_embed.proj.weight", "blocks.0.attn.qkv.weight", "blocks.11.mlp.fc2.bias", "norm.weight"):
        assert k in keys
    assert sum(v.numel() for v in VO.make_vit(0).state_dict().values()) == 21665664      # ViT-S/16


@pytest.mark.parametrize("size", [224, 112, 74])
def test_vit_oracle_against_an_independent_implementation(size):
    """Row N1's backbone: DINO's source (facebookresearch/dino vision_transformer.py) is neither under /root/reference nor
    fetchable, so the restatement oracle/vit_oracle.DinoViT is pinned against the one independent implementation of the same
    published model that IS installed here: HuggingFace transformers.ViTModel, the class the Hub's facebook/dino-vits16
    conversion of the checkpoint instantiates.  Same weights (fused qkv split into q / k / v), fp64, CLS token after the
    final LayerNorm: patch embedding, position table, 12 pre-norm blocks, 6-head attention, exact-erf GELU, eps 1e-6.
    112 and 74 are the 1/2 and 1/3 scales of the multi-scale wrapper (image_feature_extractor.py:71-87): there the position
    grid is resampled by DINO's published rule (scale factor (size + 0.1) / 14), restated in DinoViT and handed to HF as its
    table -- that one rule and the trained weights are what stays unpinned offline."""
    transformers = pytest.importorskip("transformers")
    from oracle import vit_oracle as VO
    if not hasattr(transformers, "ViTModel"):
        pytest.skip("transformers without ViTModel")
    net = VO.make_vit(seed=3, dtype=torch.float64)
    hf = VO.to_hf_vit(net, img_size=size)
    x = torch.randn(2, 3, size, size, dtype=torch.float64, generator=torch.Generator().manual_seed(size))
    with torch.no_grad():
        ours = net(x)
        theirs = hf(pixel_values=x).last_hidden_state[:, 0]
    assert tuple(ours.shape) == (2, 384)
    rel = ((ours - theirs).abs().max() / theirs.abs().max()).item()
    assert rel < 1e-12, rel


@pytest.mark.parametrize("fname", ["guided_free", "guided_free_full", "guided_free_full_s12"])
def test_free_running_fixtures_are_self_consistent(golden, fname):
    """The free-running GGS-on fixtures (reference fp32 run + fp64 oracle run, oracle/make_golden.py make_guided_free):
    the stored final mean Sampson errors are what the oracle evaluates at the stored poses on the stored matches, the
    noise tensor follows the reference's draw order (no noise on guided steps), and the full-size one is BASELINE
    configs[2] exactly (20 frames, 190 pairs x 300 matches, 10 guided steps)."""
    g = golden[fname]
    cond_start = int(g["cond_start_step"])
    shape = tuple(int(v) for v in g["img_shape"])
    for s in g["seeds"].tolist():
        if f"s{s}_kp1" in g:
            kp1, kp2, i12 = g[f"s{s}_kp1"], g[f"s{s}_kp2"], g[f"s{s}_i12"]
        else:       # round 5: seeds 1 and 2 of the full-size case store the sha256 of their matches, which are rebuilt from the stored model mean + seed
            from oracle.make_golden import regenerate_matches
            md = regenerate_matches(g, s)
            kp1, kp2, i12 = md["kp1"], md["kp2"], md["i12"]
            key = i12[:, 0] * 20 + i12[:, 1]
            assert len(key) == 57000 and len(np.unique(key)) == 190 and (np.bincount(key)[np.unique(key)] == 300).all()
        pm = O.prepare_matches(kp1, kp2, i12, shape)
        for tag in ("32", "64"):
            v, _ = O.compute_sampson_distance(torch.from_numpy(g[f"s{s}_pose{tag}"]).double(), pm)
            mean, n = g[f"s{s}_sampson{tag}"]
            assert len(v) == int(n) and abs(float(v.mean()) - mean) <= 1e-12 * max(1.0, mean)
        noise = g[f"s{s}_noise"]
        assert noise.shape[0] == 101 and not noise[101 - cond_start:].any() and noise[1:101 - cond_start].any()
        assert int(g[f"s{s}_ref_optimize_calls"]) == 5 * cond_start
    if fname == "guided_free_full":
        assert shape == (20, 3, 224, 224) and cond_start == 10
        key = g["s0_i12"][:, 0] * 20 + g["s0_i12"][:, 1]
        assert len(key) == 57000 and len(np.unique(key)) == 190 and (np.bincount(key)[np.unique(key)] == 300).all()


def test_reference_in_place_timing_fixture_is_self_consistent():
    """tests/golden/ref_timing.json (python -m oracle.make_ref_timing, where /root/reference is mounted): the reference files executed in
    place and the oracle port timed by bench.cpu_baseline on ONE host.  bench.py on the GPU box can only report the port
    (`cpu_baseline.kind == "port"`); this fixture says how the port relates to the reference itself.  Checked here: both legs are there,
    each leg's sequences/s is the extrapolation bench.py documents (100 denoiser steps + 10 x (400 all + 100 FL + 100 R + 100 T)
    iterations) of its own per-step figures, and the port is within a factor of two of the reference on every figure."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_timing.json")) as f:
        d = json.load(f)
    assert set(d["legs"]) == {"reference", "port"} and d["host_cores"] >= 1
    for kind, leg in d["legs"].items():
        g = leg["ggs_ms_per_iteration"]
        t_seq = 100 * leg["denoiser_ms_per_step"] + 10 * (400 * g["all"] + 100 * g["fl"] + 100 * g["r"] + 100 * g["t"])
        assert abs(1e3 / t_seq - leg["sequences_per_s"]) <= 0.03 * leg["sequences_per_s"], (kind, t_seq, leg["sequences_per_s"])   # (ms rounded to 0.1)
        assert ("reference files executed in place" in leg["sample"]) == (kind == "reference")
        assert leg["threads"] <= d["host_cores"]
    for k, v in d["port_over_reference"].items():
        assert 0.5 <= v <= 2.0, (k, v)
