"""GPU (-m gpu): an engine's results do not depend on its earlier calls.

One rule for every step of every script of tests/engine_history_cases.py: the result on the long-lived engine equals, bit for bit, the
result of the same call on a fresh engine of the same capacity, weights and option values that has run nothing else.  What could make
them differ is what a ``pd_engine`` keeps between calls: the activation workspaces (rows >= M left from a larger call, shared by the
four paths), the generic path's padded arrays, zproj, d_t_row, the frame counts, the three denoiser options, the sticky asynchronous
error word and the hipGraph cache of pd_sample_phase with its key and LRU eviction.

  A  step-level calls at the default shape on one engine for 64 sequences, in segments; anchored to fp64 at its end
  B  graph cache on the small path: PD_GRAPH_CACHE_MAX + 3 keys, every key visited twice, against eager launches of fresh engines
  C  the same on the large paths, where a key that forgot an option replays another mode's launches
  D  the shape-generic path (the zero padding columns of DESIGN 3.5)
"""
import pytest
import torch

import engine_history_cases as E
from conftest import rel_err
from posediffusion_amd.engine import PoseEngine
from posediffusion_amd.host import denoiser_state
from posediffusion_amd.schedule import diffusion_buffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5                    # one denoiser evaluation against fp64, as everywhere in the suite
Z_DIM = 384


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.nan_to_num(nan=-7.0, posinf=-8.0, neginf=-9.0), b.nan_to_num(nan=-7.0, posinf=-8.0, neginf=-9.0))


def assert_bitwise(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), (what, f"output {i}", f"{int((g != w).sum())} of {g.numel()} values differ")


def assert_nan_stays_in_its_sequence(nan_out, clean_out, step, what):
    """The sequence whose x is NaN comes back non-finite; every other sequence is bitwise the clean call's."""
    s = step["nan_seq"]
    others = [b for b in range(step["B"]) if b != s]
    for n, c in zip(nan_out, clean_out):
        assert not torch.isfinite(n[s]).any(), (what, "the NaN sequence holds finite values")
        assert torch.isfinite(c).all(), what
        assert torch.equal(n[others], c[others]), (what, "a NaN sequence changed another sequence")


@pytest.fixture(scope="module")
def default_sd(seeded_diffuser):
    return {k: v.detach().cpu().clone() for k, v in denoiser_state(seeded_diffuser.model).items()}


@pytest.fixture(scope="module")
def sd64(oracle_weights):
    return {k: v.double() for k, v in oracle_weights.items()}


def _engine(sd, tables, cap, **kw):
    return PoseEngine(sd, tables, device=torch.device(DEV), max_B=cap[0], max_N=cap[1], **kw)


def _fresh_result(make, step, inp, has_streamed, use_graph):
    eng = make()
    try:
        if step["scene"]:
            E.upload_scene(eng, step["scene"])
        out = [t.clone() for t in E.run_step(eng, step, inp, has_streamed, use_graph=use_graph)]
        torch.cuda.synchronize()
        return eng, out
    except Exception:
        eng.close()
        raise


# ---- A ---------------------------------------------------------------------------------------------------------------------------------
def _fp64_anchor(sd64, step, inp, out, sub):
    from oracle import pd_oracle as O
    with torch.no_grad():
        ref = O.denoiser_forward(sd64, inp["x"][sub].double(), torch.full((len(sub),), step["t"], dtype=torch.long), inp["z"][sub].double())
    return rel_err(out[sub], ref)


@pytest.mark.parametrize("seg", range(len(E.A_SEGMENTS)))
def test_a_step_level_calls_are_bitwise_a_fresh_engines(seg, default_sd, sd64):
    """Script A, steps [lo, hi) of this segment checked; the steps before them run on the long-lived engine unchecked, so that every
    segment sees the whole history.  The last small-path and the last fp16-plane step are also held to fp64 (figures in
    profiles/engine_history.txt)."""
    lo, hi = E.A_SEGMENTS[seg]
    tables = diffusion_buffers(timesteps=E.A_TIMESTEPS)
    make = lambda: _engine(default_sd, tables, E.A_CAP)
    paths = [E.path_of(s, E.A_CAP) for s in E.SCRIPT_A]
    anchors = {max(i for i, p in enumerate(paths) if p == path): path for path in (E.SMALL, E.F16_PLANES)}
    eng = make()
    try:
        outs = []
        for i, step in enumerate(E.SCRIPT_A[:hi]):
            inp = E.draw_inputs(step, Z_DIM, E.A_TIMESTEPS)
            outs.append([t.clone() for t in E.run_step(eng, step, inp, True)])
            if i < lo:
                continue
            what = f"script A step {i} ({step['kind']} {step['B']} x {step['N']}, {paths[i]})"
            fresh, want = _fresh_result(make, step, inp, True, True)
            try:
                assert_bitwise(outs[i], want, what)
                if step["nan_pair"]:
                    assert_nan_stays_in_its_sequence(outs[i - 1], outs[i], E.SCRIPT_A[i - 1], what)
                if i in anchors:
                    B = step["B"]
                    sub = sorted({0, B // 2, B - 1})
                    e = _fp64_anchor(sd64, step, inp, outs[i][0], sub)
                    print(f"fp64 anchor, step {i} ({paths[i]}, {B} x {step['N']}): rel_err {e:.2e}")
                    assert e < TOL, (what, e)
                    if anchors[i] == E.F16_PLANES:         # planes within 2 x the exact mode's own error
                        e0 = _fp64_anchor(sd64, step, inp, E.run_step(fresh, dict(step, split=0), inp, True)[0], sub)
                        print(f"fp64 anchor, step {i}: exact fp32 mode rel_err {e0:.2e}")
                        assert e0 < TOL and e <= max(2.0 * e0, 2e-6), (what, e, e0)
            finally:
                fresh.close()
        eng.check_async()                                   # nothing sticky is left behind
        if hi == len(E.SCRIPT_A):
            assert E.SCRIPT_A[-1] == E.SCRIPT_A[0]
            assert_bitwise(outs[-1], outs[0], "script A: the first call repeated at the end")
    finally:
        eng.close()


# ---- B, C ------------------------------------------------------------------------------------------------------------------------------
def _run_graph_script(name, sd, timesteps):
    script, cap, _ = E.GRAPH_SCRIPTS[name]
    has_streamed = cap[0] * cap[1] >= E.PD_STREAM_MIN_ROWS
    tables = diffusion_buffers(timesteps=timesteps)
    make = lambda: _engine(sd, tables, cap)
    events = iter(E.simulate_cache(script))
    refs = {}
    eng = make()
    try:
        for i, step in enumerate(script):
            if step["kind"] == "matches":
                E.upload_scene(eng, step["scene"])
                continue
            inp = E.draw_inputs(step, Z_DIM, timesteps)
            got = E.run_step(eng, step, inp, has_streamed, use_graph=True)
            ev = [next(events)[1] for _ in E.graph_keys(step)]
            sid = E.step_id(step)
            if sid not in refs:                             # eager launches of an engine that has run nothing else
                fresh, refs[sid] = _fresh_result(make, step, inp, has_streamed, False)
                fresh.close()
            assert len(got) == (3 if step["scene"] else 2)
            assert_bitwise(got, refs[sid], f"script {name} step {i} ({step['B']} x {step['N']}, graph {'/'.join(ev)}, "
                                           f"{E.path_of(step, cap)}, options {step['split']}/{step['fused']}/{step['long']}, "
                                           f"counts {'set' if step['counts'] else 'not set'}, cond_start {step['cond_start']})")
            assert torch.isfinite(got[0]).all()
        eng.check_async()
    finally:
        eng.close()


def test_b_graph_cache_small_path_eviction_and_replay(default_sd):
    """11 keys on an engine of 4 x 10: shapes, long-attn, counts, the fused option, guided at two cond_start values, one split call;
    then every key again in another order (7 recaptured after eviction, 4 replayed).  Every pose, process and stats tensor bitwise the
    eager result of a fresh engine."""
    _run_graph_script("B", default_sd, E.B_TIMESTEPS)


def test_c_graph_cache_large_paths_every_option_in_the_key(default_sd):
    """11 keys at 52 x 20 = 1 040 rows on an engine of 52 x 40: the three split modes, fused 0 / 2, long-attn, counts, (26, 40), (3, 20) on the
    small path unguided and guided, a second z at a cached key.  A key without one of the options replays the other mode's launches:
    modes 0 and 2, the MFMA and the key-tiled attention differ at rounding level, which the bitwise comparison sees."""
    _run_graph_script("C", default_sd, E.C_TIMESTEPS)


# ---- D ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", (0, 1), ids=("d32_padded", "post_norm_no_pivot"))
def test_d_generic_path_is_bitwise_a_fresh_engines(which):
    from denoiser_cfgs import build_dropin
    cfg = E.d_configs()[which]
    den = build_dropin(cfg, seed=90 + which)
    sd = {k: v.detach().clone() for k, v in denoiser_state(den).items()}
    tables = diffusion_buffers(timesteps=E.D_TIMESTEPS)
    make = lambda: _engine(sd, tables, E.D_CAP, num_layers=cfg.layers, nhead=cfg.heads, norm_first=cfg.norm_first, pivot=cfg.pivot)
    eng = make()
    try:
        outs = []
        for i, step in enumerate(E.SCRIPT_D):
            inp = E.draw_inputs(step, cfg.z, E.D_TIMESTEPS)
            outs.append([t.clone() for t in E.run_step(eng, step, inp, False, use_graph=True)])
            what = f"script D ({cfg.name}) step {i} ({step['kind']} {step['B']} x {step['N']})"
            fresh, want = _fresh_result(make, step, inp, False, step["kind"] != "sample")      # the sampler: eager on the fresh engine
            fresh.close()
            assert_bitwise(outs[i], want, what)
            if step["nan_pair"]:
                assert_nan_stays_in_its_sequence(outs[i - 1], outs[i], E.SCRIPT_D[i - 1], what)
            elif step["nan_seq"] is None and step["counts"] is None:
                assert all(torch.isfinite(t).all() for t in outs[i]), what
        eng.check_async()
        assert_bitwise(outs[-1], outs[0], "script D: the first call repeated at the end")
    finally:
        eng.close()
