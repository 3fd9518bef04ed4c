"""What a ``pd_engine`` carries from one call to the next, as scripts: ordered lists of calls on ONE engine whose every result must be
bitwise the result of the same call on a fresh engine (tests/test_gpu_engine_history.py; the scripts' own claims are asserted on the CPU
by tests/test_engine_history_cpu.py).  Importable without a GPU.

A step is a plain dict (``_step`` lists the fields): a kind, a shape, seeds, the three denoiser options in force, frame counts, and for
the sampler the guided part.  ``draw_inputs`` draws a step's tensors from its seed, ``run_step`` runs it on a given engine.

Restated from the library, with the lines restated:
  * ``den_plan``: pd_den_step_plan (posediffusion_amd/csrc/pd_denoiser_plan.h:37-65) with pd_qkv_attn_group / pd_qkv_attn_wgs
    (pd_qkv_attn.h:35-40) -- which kernels one denoiser evaluation launches;
  * ``graph_keys``: pd_engine::GraphKey (pd_internal.h:302-306) as pd_sample_phase fills it (pd_engine.hip:663-680) and compares it
    (:684-686); ``simulate_cache`` its 8-entry LRU (:682-714).
"""
from __future__ import annotations

import os
import re
from collections import namedtuple
from typing import Dict, List

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_INTERNAL_H = os.path.join(ROOT, "posediffusion_amd", "csrc", "pd_internal.h")


def _define(path: str, name: str) -> int:
    with open(path) as fh:
        m = re.search(r"^#define\s+" + name + r"\s+(\d+)\s*$", fh.read(), re.M)
    if not m:
        raise RuntimeError(f"{name} not found in {path}")
    return int(m.group(1))


PD_GRAPH_CACHE_MAX = _define(_INTERNAL_H, "PD_GRAPH_CACHE_MAX")
PD_STREAM_MIN_ROWS = _define(os.path.join(ROOT, "posediffusion_amd", "csrc", "pd_gemm_stream.h"), "PD_STREAM_MIN_ROWS")
PD_QA_ROWS, NH = 96, 4              # pd_qkv_attn.h (whole sequences in at most 95 token rows); heads of the default shape
CUS = 256                           # MI355X; pd_den_step_plan's own default when the device reports none (:51)

SMALL, STREAMED, BF16_PLANES, F16_PLANES = "small", "streamed", "bf16_planes", "f16_planes"      # enum PdDenPath (:13-18)
PATHS = (SMALL, STREAMED, BF16_PLANES, F16_PLANES)


def den_plan(B: int, N: int, split: int, fused: int, long: int, ragged: bool, has_streamed: bool, cus: int = CUS) -> Dict:
    """pd_den_step_plan: the path and the attention form of one evaluation.  The planes of a split mode are built when the mode is set
    (pd_engine_set_option), so ``split_ready`` / ``split_h_ready`` hold whenever the mode is in force."""
    M = B * N
    long_attn = N > 64 or long != 0 or ragged                                                     # :42
    if M < PD_STREAM_MIN_ROWS or not has_streamed:                                                # :46
        path = SMALL
    elif split == 2:                                                                              # :47
        path = F16_PLANES
    elif split == 1:                                                                              # :48
        path = BF16_PLANES
    else:
        path = STREAMED
    p = {"path": path, "rows": M, "long_attn": long_attn, "fused_attn": False, "attn_mma": False}
    if path != F16_PLANES:                                                                        # :50
        return p
    G = (PD_QA_ROWS - 1) // N if 1 <= N <= 32 else 0                                              # pd_qkv_attn.h:35
    qa_wgs = ((B + G - 1) // G) * NH if G else 0                                                  # pd_qkv_attn.h:37-40
    qa_fills = 4 * qa_wgs >= 3 * ((qa_wgs + cus - 1) // cus) * cus                                # :55
    p["fused_attn"] = qa_wgs > 0 and not long_attn and (qa_fills if fused == 1 else fused == 2)   # :56
    p["attn_mma"] = N <= 32 and not long_attn                                                     # :57 (the knob is 1 in the product build)
    return p


# ---- steps ---------------------------------------------------------------------------------------------------------------------------
KINDS = ("denoise", "p_mean_finish", "denoise_t", "p_losses", "sample", "matches")
_DEFAULTS = dict(t=42, split=0, fused=1, long=0, counts=None, nan_seq=None, nan_pair=False, bad_t=False, loss_type="l1",
                 cond_start=0, scene=None, phases="all")


def _step(kind: str, B: int = 0, N: int = 0, seed: int = 0, **kw) -> Dict:
    """kind; (B, N); seed of the inputs; t: one timestep, or one per sequence (denoise_t, p_losses); split / fused / long: the values of
    PD_OPT_DENOISER_SPLIT / _FUSED_ATTN / _LONG_ATTN in force; counts: frame counts per sequence or None; nan_seq: the sequence whose x
    is NaN in all rows; nan_pair: this is the clean call of the NaN step before it (same seed); bad_t: t holds an entry outside
    [0, timesteps); sample only -- cond_start, scene (the name of the match scene: guided) and phases ("all": one call, "split": phase 1
    then phase 2)."""
    assert kind in KINDS and not set(kw) - set(_DEFAULTS), (kind, kw)
    return dict(_DEFAULTS, kind=kind, B=B, N=N, seed=seed, **kw)


def step_id(step: Dict):
    """Hashable identity of a step: two steps with one id are the same call on the same inputs (they share one fresh-engine reference)."""
    return tuple((k, tuple(v) if isinstance(v, list) else v) for k, v in sorted(step.items()))


GGS_ITERS = 5
SCENES = {"b2n8": dict(B=2, N=8, seed=4100, per_pair=40), "b3n20": dict(B=3, N=20, seed=4200, per_pair=40)}
_MATCHES: Dict[str, list] = {}


def scene_matches(name: str):
    """synth.make_matches scenes, one per sequence slot (built once per process)."""
    if name not in _MATCHES:
        from posediffusion_amd import synth
        sc = SCENES[name]
        _MATCHES[name] = [synth.make_matches(synth.make_cameras(sc["N"], seed=sc["seed"] + b), 224, 224, per_pair=sc["per_pair"],
                                             seed=sc["seed"] + b) for b in range(sc["B"])]
    return _MATCHES[name]


def upload_scene(eng, name: str):
    for b, md in enumerate(scene_matches(name)):
        eng.set_matches(b, md["kp1"], md["kp2"], md["i12"], md["img_shape"])


def ggs_cfg():
    from posediffusion_amd import synth
    return dict(synth.GGS_CFG, iter_num=GGS_ITERS)


def draw_inputs(step: Dict, z_dim: int, timesteps: int) -> Dict[str, torch.Tensor]:
    """CPU tensors of a step, from its seed alone."""
    B, N = step["B"], step["N"]
    g = torch.Generator().manual_seed(step["seed"])
    d = {"x": torch.randn(B, N, 9, generator=g), "z": torch.randn(B, N, z_dim, generator=g), "noise": torch.randn(B, N, 9, generator=g)}
    if step["kind"] == "sample":
        d["noise"] = torch.randn(timesteps + 1, B, N, 9, generator=g)
    if step["nan_seq"] is not None:
        d["x"][step["nan_seq"]] = float("nan")
    if step["kind"] in ("denoise_t", "p_losses"):
        d["t"] = torch.tensor(step["t"], dtype=torch.int64)
        assert d["t"].numel() == B
    return d


def set_options(eng, step: Dict, has_streamed: bool):
    """The step's option values on ``eng``.  Below PD_STREAM_MIN_ROWS rows of capacity the split modes are refused
    (pd_denoiser_build_split, pd_denoiser.hip:198-202): such an engine stays at 0."""
    from posediffusion_amd import _lib
    if has_streamed:
        eng.set_split_precision(step["split"])
    else:
        assert step["split"] == 0
    eng.set_option(_lib.PD_OPT_DENOISER_FUSED_ATTN, step["fused"])
    eng.set_option(_lib.PD_OPT_DENOISER_LONG_ATTN, step["long"])


def run_step(eng, step: Dict, inp: Dict[str, torch.Tensor], has_streamed: bool, use_graph: bool = True) -> List[torch.Tensor]:
    """One step on ``eng`` (options first): the list of its result tensors, on the device."""
    dev = eng.device
    set_options(eng, step, has_streamed)
    x, z, noise = inp["x"].to(dev), inp["z"].to(dev), inp["noise"].to(dev)
    kind, counts = step["kind"], step["counts"]
    if kind == "denoise":
        return [eng.denoise(x, z, step["t"], n_frames=counts)]
    if kind == "p_mean_finish":
        mean, x0 = eng.p_mean(x, z, step["t"], n_frames=counts)
        return [mean, x0, eng.p_finish(mean, noise if step["t"] > 0 else None, step["t"], n_frames=counts)]
    if kind in ("denoise_t", "p_losses"):
        if kind == "denoise_t":
            out = [eng.denoise_t(x, z, inp["t"].to(dev))]
        else:
            r = eng.p_losses(x, z, inp["t"].to(dev), noise, loss_type=step["loss_type"])
            out = [r[k] for k in ("loss", "x_0_pred", "x_t", "model_out")]
        if step["bad_t"]:                     # bit 3 of the sticky error word: reported once, then cleared (pd_check_async_error)
            try:
                eng.check_async()
            except RuntimeError as e:
                assert "timestep outside" in str(e), e
            else:
                raise AssertionError("an out-of-range timestep was not reported by check_async")
            eng.check_async()
        return out
    assert kind == "sample"
    guided = step["scene"] is not None
    cfg = ggs_cfg() if guided else None
    kw = dict(use_graph=use_graph, n_frames=counts)
    if step["phases"] == "split":
        out = eng.sample(z, noise, step["cond_start"], cfg, phase=1, **kw)
        out = eng.sample(z, noise, step["cond_start"], cfg, phase=2, out=out, **kw)
    else:
        out = eng.sample(z, noise, step["cond_start"], cfg, **kw)
    if guided:
        eng.check_async()
    return [t for t in out if t is not None]


# ---- graph keys ----------------------------------------------------------------------------------------------------------------------
GraphKey = namedtuple("GraphKey", "B N cond_start has_ggs phase split fused long counts_set cfg plan")
KEY_OPTION_FIELDS = ("split", "fused", "long", "counts_set", "cond_start")


def graph_keys(step: Dict) -> List[GraphKey]:
    """The keys a ``sample`` step looks up, in order.  B, N, cond_start (0 unless guided), has_ggs, phase; the options packed into
    GraphKey::den_split (split | fused << 8 | long << 16 | counts set << 24, pd_engine.hip:670); the GGS configuration (guided only) and
    the match-derived plan (guided, phases 0 and 2 only, :673-679) -- here the scene's name, as one scene gives one plan."""
    assert step["kind"] == "sample"
    has_ggs = step["scene"] is not None and step["cond_start"] > 0
    keys = []
    for phase in ((1, 2) if step["phases"] == "split" else (0,)):
        keys.append(GraphKey(step["B"], step["N"], step["cond_start"] if has_ggs else 0, has_ggs, phase, step["split"], step["fused"],
                             step["long"], step["counts"] is not None, GGS_ITERS if has_ggs else None,
                             step["scene"] if has_ggs and phase != 1 else None))
    return keys


def differ_only_in(a: GraphKey, b: GraphKey, field: str) -> bool:
    return getattr(a, field) != getattr(b, field) and all(getattr(a, f) == getattr(b, f) for f in GraphKey._fields if f != field)


def simulate_cache(steps: List[Dict], cap: int = PD_GRAPH_CACHE_MAX):
    """[(key, event)] over the script: "capture" (first sight), "replay" (found), "recapture" (seen before, evicted since).  Most
    recently used last; the front goes when a capture finds ``cap`` entries (pd_engine.hip:688, :708-713)."""
    cache, seen, events = [], set(), []
    for st in steps:
        if st["kind"] != "sample":
            continue
        for k in graph_keys(st):
            if k in cache:
                cache.remove(k)
                cache.append(k)
                events.append((k, "replay"))
                continue
            if len(cache) >= cap:
                cache.pop(0)
            cache.append(k)
            events.append((k, "recapture" if k in seen else "capture"))
            seen.add(k)
    return events


# ---- script A: step-level calls on one engine of 64 sequences (default shape) -----------------------------------------------------------
# max_N = 64 so that (20, 64) fits the engine that also takes (64, 20): the workspaces hold 64 x 64 rows, every call uses at most 1 280.
A_CAP = (64, 64)
A_TIMESTEPS = 100
_L = dict(split=2)            # an engine with the streamed path starts in the fp16-plane mode (pd_engine.hip:322-324)
_T64 = [(7 * b + 3) % 100 for b in range(64)]
_UNEVEN52 = [1 + (b * 7) % 20 for b in range(52)]
SCRIPT_A = [
    # every ordered pair of paths: f16 -> small -> streamed -> small -> bf16 -> f16 -> streamed -> f16 -> bf16 -> streamed -> bf16 -> small -> f16
    _step("denoise", 64, 20, 100, split=2, fused=1),                                    # 0  f16 planes (the script ends on this call again)
    _step("denoise", 3, 20, 101, **_L),                                                 # 1  small: rows 60 .. 1279 are the call's before
    _step("denoise", 64, 20, 102, split=0),                                             # 2  streamed, exact fp32
    _step("denoise", 2, 7, 103, split=0, t=0),                                          # 3  small
    _step("p_mean_finish", 64, 20, 104, split=1, t=99),                                 # 4  bf16 planes
    _step("denoise", 64, 20, 105, split=2, fused=0),                                    # 5  f16 planes, two-launch attention
    _step("p_losses", 64, 20, 106, split=0, t=_T64),                                    # 6  streamed, one t per sequence
    _step("denoise", 64, 20, 107, split=2, fused=2),                                    # 7  f16 planes, fused in_proj + attention
    _step("denoise_t", 64, 20, 108, split=1, t=_T64[::-1]),                             # 8  bf16 planes, distinct t (d_t_row) ...
    _step("denoise", 64, 20, 109, split=0, t=5),                                        # 9  ... then one t, streamed
    _step("denoise", 40, 32, 110, split=1),                                             # 10 bf16 planes, N = 32
    _step("denoise", 51, 20, 111, **_L),                                                # 11 small at 1 020 rows of the large engine
    _step("denoise", 40, 32, 112, split=2, fused=2),                                    # 12 f16 planes, fused at N = 32
    # 33 .. 64 frames: no fused kernel, no MFMA attention
    _step("denoise", 20, 64, 113, split=2),                                             # 13
    _step("denoise", 20, 64, 114, split=0),                                             # 14
    _step("p_mean_finish", 40, 32, 115, split=2, t=0),                                  # 15 (t = 0: p_finish without noise)
    # long-attn 1, then 0
    _step("denoise", 64, 20, 116, split=2, long=1),                                     # 16
    _step("denoise", 64, 20, 117, split=2, long=0),                                     # 17
    _step("denoise", 3, 20, 118, split=2, long=1),                                      # 18
    _step("denoise", 3, 20, 119, split=2, long=0),                                      # 19
    # counts set (uneven), cleared, the uniform call
    _step("denoise", 52, 20, 120, split=2, counts=_UNEVEN52),                           # 20
    _step("denoise", 52, 20, 121, split=2),                                             # 21
    _step("p_mean_finish", 3, 20, 122, split=2, counts=[20, 1, 13]),                    # 22
    _step("denoise", 3, 20, 123, split=2),                                              # 23
    # an out-of-range t: reported once by check_async, then gone
    _step("denoise_t", 64, 20, 124, split=2, t=[100] + _T64[1:], bad_t=True),           # 24
    _step("denoise", 64, 20, 125, split=2, t=7),                                        # 25
    # NaN in all rows of one sequence, then the clean call, on every path
    _step("denoise", 64, 20, 126, split=2, nan_seq=17),                                 # 26
    _step("denoise", 64, 20, 126, split=2, nan_pair=True),                              # 27
    _step("denoise", 64, 20, 127, split=0, nan_seq=63),                                 # 28
    _step("denoise", 64, 20, 127, split=0, nan_pair=True),                              # 29
    _step("denoise", 64, 20, 128, split=1, nan_seq=0),                                  # 30
    _step("denoise", 64, 20, 128, split=1, nan_pair=True),                              # 31
    _step("denoise", 3, 20, 129, split=2, nan_seq=1),                                   # 32
    _step("denoise", 3, 20, 129, split=2, nan_pair=True),                               # 33
    _step("denoise", 64, 20, 130, split=2, fused=2, nan_seq=31),                        # 34 the fused kernel holds 4 sequences per workgroup
    _step("denoise", 64, 20, 130, split=2, fused=2, nan_pair=True),                     # 35
    _step("p_losses", 3, 20, 131, split=2, t=[0, 99, 50], loss_type="l2"),              # 36
    _step("denoise", 51, 20, 132, split=2),                                             # 37 the last small step (fp64 anchor)
    _step("denoise", 64, 20, 100, split=2, fused=1),                                    # 38 = step 0, the last f16-plane step (fp64 anchor)
]
A_SEGMENTS = [(0, 10), (10, 20), (20, 30), (30, len(SCRIPT_A))]


def path_of(step: Dict, cap) -> str:
    has_streamed = cap[0] * cap[1] >= PD_STREAM_MIN_ROWS                 # den_create_activations, pd_denoiser.hip:110
    return den_plan(step["B"], step["N"], step["split"], step["fused"], step["long"], step["counts"] is not None, has_streamed)["path"]


def _other_inputs(step: Dict) -> Dict:
    """The same call (the same graph key) on other inputs: a revisit whose replay did nothing could not pass."""
    return dict(step, seed=step["seed"] + 50)


# ---- script B: graph cache on the small path, capacity 4 x 10, 6 timesteps ------------------------------------------------------------------
B_CAP = (4, 10)
B_TIMESTEPS = 6
_B_KEYS = {
    "b4n10": _step("sample", 4, 10, 200),
    "b2n10": _step("sample", 2, 10, 201),
    "b3n7": _step("sample", 3, 7, 202),
    "b1n1": _step("sample", 1, 1, 203),
    "b4n10_long": _step("sample", 4, 10, 204, long=1),
    "b4n10_counts": _step("sample", 4, 10, 205, counts=[10, 4, 7, 1]),
    "b4n10_fused2": _step("sample", 4, 10, 206, fused=2),
    "g_cs2": _step("sample", 2, 8, 207, scene="b2n8", cond_start=2),
    "g_cs3": _step("sample", 2, 8, 208, scene="b2n8", cond_start=3),
    "g_cs2_split": _step("sample", 2, 8, 209, scene="b2n8", cond_start=2, phases="split"),       # two keys: phase 1, phase 2
}
_B_FIRST = ["b4n10", "b2n10", "b3n7", "b1n1", "b4n10_long", "b4n10_counts", "b4n10_fused2", "g_cs2", "g_cs3", "g_cs2_split"]
_B_AGAIN = ["g_cs3", "b4n10", "b4n10_counts", "b2n10", "g_cs2_split", "b3n7", "b4n10_long", "g_cs2", "b4n10_fused2", "b1n1"]
SCRIPT_B = [_step("matches", scene="b2n8")] + [_B_KEYS[k] for k in _B_FIRST] + [_other_inputs(_B_KEYS[k]) for k in _B_AGAIN]
B_FIELDS = ("fused", "long", "counts_set", "cond_start")          # split: refused below 1 024 rows of capacity (set_options)

# ---- script C: graph cache on the large paths, calls of 52 x 20 = 1 040 rows, 4 timesteps ------------------------------------------------
C_CAP = (52, 40)              # max_N = 40 for (26, 40); every call is 1 040 rows or fewer
C_TIMESTEPS = 4
_C_KEYS = {
    "split2": _step("sample", 52, 20, 300, split=2),
    "split0": _step("sample", 52, 20, 301, split=0),
    "split1": _step("sample", 52, 20, 302, split=1),
    "fused0": _step("sample", 52, 20, 303, split=2, fused=0),
    "fused2": _step("sample", 52, 20, 304, split=2, fused=2),
    "long1": _step("sample", 52, 20, 305, split=2, long=1),
    "counts": _step("sample", 52, 20, 306, split=2, counts=_UNEVEN52),
    "b26n40": _step("sample", 26, 40, 307, split=2),
    "b3n20": _step("sample", 3, 20, 308, split=2),
    "g_cs1": _step("sample", 3, 20, 309, split=2, scene="b3n20", cond_start=1),
    "g_cs2": _step("sample", 3, 20, 310, split=2, scene="b3n20", cond_start=2),
    "split2_z2": _step("sample", 52, 20, 311, split=2),           # the key of "split2" with another z: zproj is per call
}
_C_FIRST = ["split2", "split2_z2", "split0", "split1", "fused0", "fused2", "long1", "counts", "b26n40", "b3n20", "g_cs1", "g_cs2"]
_C_AGAIN = ["g_cs2", "split0", "long1", "split2", "split2_z2", "counts", "fused2", "split1", "b3n20", "fused0", "g_cs1", "b26n40"]
SCRIPT_C = [_step("matches", scene="b3n20")] + [_C_KEYS[k] for k in _C_FIRST] + [_other_inputs(_C_KEYS[k]) for k in _C_AGAIN]
C_FIELDS = KEY_OPTION_FIELDS
GRAPH_SCRIPTS = {"B": (SCRIPT_B, B_CAP, B_FIELDS), "C": (SCRIPT_C, C_CAP, C_FIELDS)}

# ---- script D: the shape-generic path, capacity 3 x 8, 6 timesteps ------------------------------------------------------------------------
D_CAP = (3, 8)
D_TIMESTEPS = 6
SCRIPT_D = [
    _step("denoise", 1, 3, 400, t=5),
    _step("denoise", 3, 8, 401, t=0),
    _step("denoise", 2, 5, 402, t=3),
    _step("p_mean_finish", 3, 8, 403, t=4),
    _step("denoise", 3, 8, 404, t=2, counts=[8, 3, 1]),
    _step("denoise", 3, 8, 405, t=2),
    _step("denoise", 3, 8, 406, t=1, nan_seq=1),
    _step("denoise", 3, 8, 406, t=1, nan_pair=True),
    _step("denoise_t", 2, 5, 407, t=[5, 0]),
    _step("sample", 2, 5, 408),
    _step("sample", 3, 8, 409),
    _step("denoise", 1, 1, 410, t=3),
    _step("sample", 2, 5, 411),                                   # replayed, other inputs
    _step("sample", 3, 8, 412, counts=[2, 8, 5]),
    _step("p_losses", 3, 8, 413, t=[0, 5, 2]),
    _step("denoise", 1, 3, 400, t=5),                             # the first call again
]


def d_configs():
    """EDGE_CFGS[0] (d = 32: Dp = 64, 32 padding columns) and a post-norm, no-pivot configuration."""
    from denoiser_cfgs import CONFIGS, EDGE_CFGS
    post = [c for c in CONFIGS if not c.norm_first and not c.pivot]
    return [EDGE_CFGS[0], post[0]]
