"""Scenes, optimiser settings and fp64 / fp32 oracle references of the GGS input-domain tests (a plain helper module, imported by
tests/test_ggs_inputs_cpu.py, tests/test_gpu_ggs_inputs.py and tests/test_oracle_golden.py).  oracle/make_golden.py does not import it: it
states the fixture scene and its three (alpha, learning_rate) pairs itself (GGS_INPUTS_SCENE / GGS_INPUTS_SETTINGS) and stores them in
tests/golden/ggs_inputs.npz; test_oracle_golden.py and the GPU fixture test assert that the stored scene and settings equal the ones here.

Two inputs the rest of the suite keeps constant are varied here:

  * the image shape.  At a square image sc = min(H, W) / 2, cx = W / 2 and cy = H / 2 are one number.  sc equals the smaller of cx and cy
    by definition, so one non-square shape separates only two of the three: at 192 x 320 sc = cy = 96, cx = 160; at 320 x 192 sc = cx = 96,
    cy = 160.  Both orientations together tell all three apart, which is why every kernel family runs both.
  * (alpha, learning_rate, momentum).  With the defaults coef = min(alpha |x_masked| / (lr (|g| + 1e-6)), 1) is 1e-3 .. 1e-1: the step is
    alpha |x_masked| g / |g|, in which learning_rate and every common factor of g cancel.  SETTINGS adds a never-clipped setting
    (coef == 1 in every iteration), one that crosses between clipped and unclipped, learning_rate alone changed, and momentum 0.5 / 0.0.

What was fixed on the CPU oracle, and why:

  * "crossing" takes (alpha, learning_rate) per scene (CROSSING): the all-groups stage has iterations on both sides of the clip, and the
    UNCLAMPED ratio alpha |x_masked| / (lr (|g| + 1e-6)) is more than 1 % away from 1 in every iteration of every stage, in fp64 and fp32
    alike, so the engine's fp32 ratio cannot land on the other branch.  Ratios of the all-groups stage: (8, 224, 224) 1.02, 0.98, 0.95,
    1.04, 1.14, 1.10; (6, 192, 320) 0.90, 0.96, 1.06, 1.18, 1.43, 1.82; (33, 96, 512) 0.92, 1.36, 1.38, 1.40.  On the 33-frame
    192 x 320 scene the ratio moves by under 3 % over the iterations, so any crossing alpha puts an iterate within 1 % of 1 there; the
    two-hop kernel, which only 33 frames reach, gets its crossing run from the 96 x 512 scene, whose gradient drops by a third after the
    first step.  At 65 frames the all-groups stage has two iterations with ratios 2e-3 apart: no crossing there.
  * Valid counts are compared exactly at the start pose of every scene and at every iterate of the all-groups stage's trace, so no match
    may lie within BAND of sampson_max there.  On the fp64 oracle the share of iterates that hold such a match grows with the number
    of matches: seldom at 600 / 1 680 matches (6 / 8 frames), often at 8 448 (33 frames), about half of them at 16 640 (65 frames), so
    a seed that is clear over six iterations of five settings is out of reach there.  So the regimes run 2 iterations per stage at 33
    frames and 1 at 65 (REGIME_ITER_NUM; the all-groups stage then has 4 / 2 iterations, momentum acting from the second), and SEEDS holds the first seed whose compared iterates
    are clear in every setting of the scene, searched in this order: 700 + N, then 1733, 1734, ... at (33, 192, 320) -- 1974, the 243rd
    tried -- and 765, 766, ... at (65, 192, 320) -- 767.  To repeat the search: threshold_margin over scene(...)'s start pose and over
    optimize_refs(...)["trace64"][:-1] for every setting of settings_of(key).

Every reference is computed once per (scene, setting, flags) on one CPU thread and shared (functools.lru_cache); callers must not modify
what they get.  tests/test_ggs_inputs_cpu.py asserts, without a GPU, the conditions the GPU tests rest on: the regimes, the distance of
every Sampson value from sampson_max at every compared iterate, and that the checks see the errors they are for.
"""
import functools

import torch

import ggs_checks as G
from oracle import pd_oracle as O
from posediffusion_amd import synth

SAMPSON_MAX = 10.0
BAND = 1e-4                        # ggs_checks.sampson_max_for's contract band (relative)
SHAPES = {"192x320": (192, 320), "320x192": (320, 192), "96x512": (96, 512), "1080x1920": (1080, 1920)}
PER_PAIR = {4: 40, 5: 40, 6: 40, 8: 60, 33: 16, 65: 8}           # matches per frame pair at each frame count
FLAGS = {"all": (True, True, True), "fl": (False, False, True), "r": (True, False, False), "t": (False, True, False)}   # (R, T, FL)
ITER_NUM = 3                       # GGS_optimize iterations per stage (x 2 where all three groups update) of the image-geometry tests
REGIME_ITER_NUM = {8: 3, 6: 3, 33: 2, 65: 1}      # ... of the optimiser-regime tests, by frame count
GUIDE_ITER_NUM = 2                 # geometry_guided_sampling: [4, 2, 2, 2, 4] iterations

# (frames, H, W) -> scene seed, where it is not 700 + frames: chosen from the fp64 ORACLE's Sampson values alone, so that no match lies
# within BAND of sampson_max at any iterate a test evaluates (the precedent: seed 901 for 900 in tests/test_gpu_ggs_long.py)
SEEDS = {(33, 192, 320): 1974, (65, 192, 320): 767}

SETTINGS = {
    "default": dict(alpha=1e-4, learning_rate=1e-2),
    "never_clipped": dict(alpha=1.0, learning_rate=1e-4),
    "crossing": dict(),                            # alpha, learning_rate: CROSSING[scene]
    "lr_only": dict(alpha=1e-4, learning_rate=3e-3),
    "momentum_0.5": dict(alpha=1.0, learning_rate=1e-4, momentum=0.5),
    "momentum_0.0": dict(alpha=1.0, learning_rate=1e-4, momentum=0.0),
}
REGIME = {"default": "clipped", "lr_only": "clipped", "never_clipped": "unclipped", "momentum_0.5": "unclipped", "momentum_0.0": "unclipped",
          "crossing": "crossing"}
CROSSING = {(8, 224, 224): dict(alpha=2.65e-3, learning_rate=1e-3), (6, 192, 320): dict(alpha=3e-4, learning_rate=1e-4),
            (33, 96, 512): dict(alpha=3e-5, learning_rate=1e-4)}
FIXTURE_SCENE = (6, 192, 320)
FIXTURE_SETTINGS = ("default", "never_clipped", "crossing")          # the reference hard-codes momentum 0.9

GEOMETRY_SCENES = ([(6, h, w) for h, w in SHAPES.values()] + [(33, h, w) for h, w in SHAPES.values()] + [(65, 192, 320), (65, 320, 192)])
REGIME_SCENES = [(8, 224, 224), (6, 192, 320), (33, 192, 320), (33, 96, 512), (65, 192, 320)]
MIXED_SCENES = [(6, 224, 224), (6, 192, 320), (6, 320, 192), (5, 192, 320), (4, 320, 192)]


def settings_of(key):
    """The settings a regime scene runs."""
    if key == (33, 96, 512):                    # (only there for the two-hop kernel's crossing run)
        return ["crossing"]
    return [s for s in SETTINGS if s != "crossing" or key in CROSSING]


def cfg_of(setting, key=None, **over):
    """The GGS_cfg dict of a setting (synth.GGS_CFG with the setting's fields; "crossing" needs the scene `key`)."""
    cfg = dict(synth.GGS_CFG, **SETTINGS[setting])
    if setting == "crossing":
        cfg.update(CROSSING[key])
    return dict(cfg, **over)


def scene_seed(N, H, W):
    return SEEDS.get((N, H, W), 2000 if (N, H, W) == (8, 224, 224) else 700 + N)


@functools.lru_cache(maxsize=None)
def scene(N, H, W):
    """(matches dict, prepared matches, start pose [1, N, 9] float32).  (8, 224, 224) is the scene of tests/golden/ggs.npz."""
    seed = scene_seed(N, H, W)
    enc = synth.make_cameras(N, seed=seed)
    md = synth.make_matches(enc, H, W, per_pair=PER_PAIR[N], seed=seed)
    pm = O.prepare_matches(md["kp1"], md["kp2"], md["i12"], md["img_shape"])
    return md, pm, synth.perturb_pose(enc, seed=7)


@functools.lru_cache(maxsize=None)
def optimize_refs(key, setting, fname, iter_num=ITER_NUM):
    """{"x64", "x32": poses after GGS_optimize, "steps", "trace64", "trace32": the oracle's per-iteration traces} in fp64 and fp32."""
    _, pm, x0 = scene(*key)
    out = {}
    for name, dt in (("64", torch.float64), ("32", torch.float32)):
        tr = []
        with G.one_thread():
            x, _, steps = O.ggs_optimize(G._x(x0, dt), pm, *FLAGS[fname], trace=tr, **cfg_of(setting, key, iter_num=iter_num))
        out["x" + name], out["trace" + name], out["steps" + name] = x, tr, steps
    return out


@functools.lru_cache(maxsize=None)
def guide_refs(key, setting):
    """(fp64 pose, fp32 pose, iterations per stage in fp64) of geometry_guided_sampling with iter_num = GUIDE_ITER_NUM."""
    md, _, x0 = scene(*key)
    cfg = cfg_of(setting, key, iter_num=GUIDE_ITER_NUM)
    g64, steps = G.oracle_guide(x0, md, cfg)
    g32, steps32 = G.oracle_guide(x0, md, cfg, torch.float32)
    assert steps == steps32, (key, setting, steps, steps32)
    return g64, g32, steps


def threshold_margin(x, pm, sampson_max=SAMPSON_MAX):
    """min |s - sampson_max| / sampson_max over every match at pose x, in fp64."""
    with G.one_thread():
        s, _ = O.compute_sampson_distance(G._x(x, torch.float64), pm, sampson_max=float("inf"))
    return float((s.detach() - sampson_max).abs().min() / sampson_max)


def unclamped_ratios(trace, x0, cfg):
    """alpha |x_masked| / (lr (|g| + 1e-6)) of every iteration of an oracle trace started at x0 (coef is this ratio clamped to 1): above
    1 it says how far an unclipped iteration is from the clip, which coef == 1 does not."""
    out, prev = [], G._x(x0, trace[0]["x"].dtype)
    for t in trace:
        xn = (prev * (t["grad"].abs() > 0)).norm()
        out.append(float(cfg["alpha"] * xn / cfg["learning_rate"] / (t["gnorm"] + 1e-6)))
        prev = t["x"]
    return out
