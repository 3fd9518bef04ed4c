"""CPU: the scripts of tests/engine_history_cases.py are what they claim to be, so that a later edit cannot quietly empty them, and the
constants they restate are the library's."""
import os
import re

import pytest

import engine_history_cases as E

CSRC = os.path.join(E.ROOT, "posediffusion_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def test_restated_constants_are_the_librarys():
    assert E.PD_GRAPH_CACHE_MAX == int(re.search(r"#define\s+PD_GRAPH_CACHE_MAX\s+(\d+)", _src("pd_internal.h")).group(1)) >= 2
    assert E.PD_STREAM_MIN_ROWS == 1024
    assert re.search(r"#define\s+PD_QA_ROWS\s+%d\b" % E.PD_QA_ROWS, _src("pd_qkv_attn.h"))
    plan = _src("pd_denoiser_plan.h")
    # the path rule and the fused rule as den_plan restates them
    assert "if (p.M < PD_STREAM_MIN_ROWS || !has_streamed) p.path = PD_DEN_SMALL;" in plan
    assert "p.long_attn = N > 64 || long_attn != 0 || ragged;" in plan
    assert "4 * qa_wgs >= 3 * ((qa_wgs + cus - 1) / cus) * cus" in plan
    assert "qa_wgs > 0 && !p.long_attn && (fused_attn == 1 ? qa_fills : fused_attn == 2)" in plan
    assert [m for m in re.findall(r"^\s+(PD_DEN_\w+),?\s", plan, re.M)] == ["PD_DEN_SMALL", "PD_DEN_STREAMED", "PD_DEN_BF16_PLANES", "PD_DEN_F16_PLANES"]
    # the graph key: its fields, and the options packed into den_split
    eng = _src("pd_engine.hip")
    assert "int B, N, cond_start, has_ggs, phase, den_split;" in _src("pd_internal.h")
    assert "eng->den_split | (eng->den_fused_attn << 8) | (eng->den_long_attn << 16) | ((nf ? 1 : 0) << 24)" in eng
    assert "eng->graphs.size() >= PD_GRAPH_CACHE_MAX" in eng


def test_den_plan_at_known_shapes():
    big = dict(has_streamed=True)
    assert E.den_plan(51, 20, 2, 1, 0, False, **big)["path"] == E.SMALL                       # 1 020 rows
    assert E.den_plan(52, 20, 2, 1, 0, False, **big)["path"] == E.F16_PLANES                  # 1 040 rows
    assert E.den_plan(52, 20, 2, 1, 0, False, has_streamed=False)["path"] == E.SMALL
    assert E.den_plan(52, 20, 1, 1, 0, False, **big)["path"] == E.BF16_PLANES
    assert E.den_plan(52, 20, 0, 1, 0, False, **big)["path"] == E.STREAMED
    # fused = 1 takes the fused kernel only where its workgroups fill the chip's rounds: 256 sequences do, 64 and 103 do not
    assert E.den_plan(256, 20, 2, 1, 0, False, **big)["fused_attn"] and not E.den_plan(103, 20, 2, 1, 0, False, **big)["fused_attn"]
    assert not E.den_plan(64, 20, 2, 1, 0, False, **big)["fused_attn"] and E.den_plan(64, 20, 2, 2, 0, False, **big)["fused_attn"]
    assert E.den_plan(40, 32, 2, 2, 0, False, **big)["fused_attn"] and not E.den_plan(20, 64, 2, 2, 0, False, **big)["fused_attn"]
    for kw in (dict(long=1, ragged=False), dict(long=0, ragged=True)):                       # the key-tiled kernel: neither fused nor MFMA attention
        p = E.den_plan(64, 20, 2, 2, has_streamed=True, **kw)
        assert p["long_attn"] and not p["fused_attn"] and not p["attn_mma"]
    assert E.den_plan(20, 64, 2, 1, 0, False, **big)["attn_mma"] is False and not E.den_plan(20, 64, 2, 1, 0, False, **big)["long_attn"]


def test_script_a_visits_every_path_and_every_ordered_pair():
    paths = [E.path_of(s, E.A_CAP) for s in E.SCRIPT_A]
    assert set(paths) == set(E.PATHS)
    pairs = set(zip(paths, paths[1:]))
    want = {(a, b) for a in E.PATHS for b in E.PATHS if a != b}
    assert want <= pairs, want - pairs


def test_script_a_shapes_and_cases():
    A = E.SCRIPT_A
    max_B, max_N = E.A_CAP
    assert all(s["B"] <= max_B and s["N"] <= max_N and s["B"] * s["N"] <= 1280 for s in A)    # the issue's 64 x 20 rows, no larger call
    shapes = [(s["B"], s["N"]) for s in A]
    steps = list(zip(shapes, shapes[1:]))
    assert any(a[1] == b[1] and a[0] > b[0] for a, b in steps) and any(a[1] == b[1] and a[0] < b[0] for a, b in steps)
    Ns = {n for _, n in shapes}
    assert any(n <= 32 for n in Ns) and any(33 <= n <= 64 for n in Ns)
    assert any(n > 64 for n in Ns) or max_N <= 64
    for shape in ((3, 20), (2, 7), (51, 20), (40, 32), (20, 64)):
        assert shape in shapes
    for split in (0, 1, 2):
        assert any(s["split"] == split and (s["B"], s["N"]) == (64, 20) for s in A)
    for fused in (0, 1, 2):
        assert any(s["fused"] == fused and s["split"] == 2 and (s["B"], s["N"]) == (64, 20) for s in A)
    kinds = {s["kind"] for s in A}
    assert {"denoise", "p_mean_finish", "denoise_t", "p_losses"} <= kinds
    assert any(a["long"] == 1 and b["long"] == 0 and (a["B"], a["N"]) == (b["B"], b["N"]) for a, b in zip(A, A[1:]))
    assert any(a["kind"] == "denoise_t" and len(set(a["t"])) > 1 and b["kind"] == "denoise" for a, b in zip(A, A[1:]))
    assert any(a["counts"] and len(set(a["counts"])) > 1 and (a["B"], a["N"]) == (52, 20) and b["counts"] is None and (b["B"], b["N"]) == (52, 20)
               for a, b in zip(A, A[1:]))
    bad = [i for i, s in enumerate(A) if s["bad_t"]]
    assert bad and all(max(A[i]["t"]) >= E.A_TIMESTEPS and A[i + 1]["kind"] == "denoise" for i in bad)
    # every NaN step: one whole sequence of a batch of several, followed by its clean call; on every path
    nan = [i for i, s in enumerate(A) if s["nan_seq"] is not None]
    assert {E.path_of(A[i], E.A_CAP) for i in nan} == set(E.PATHS)
    for i in nan:
        clean = dict(A[i], nan_seq=None, nan_pair=True)
        assert A[i + 1] == clean and A[i]["B"] > 1 and 0 <= A[i]["nan_seq"] < A[i]["B"]
    assert all(A[i - 1]["nan_seq"] is not None for i, s in enumerate(A) if s["nan_pair"])
    assert A[-1] == A[0] and len(A) > 30
    # the fp64 anchors are plain denoise calls
    for path in (E.SMALL, E.F16_PLANES):
        last = [s for s in A if E.path_of(s, E.A_CAP) == path][-1]
        assert last["kind"] == "denoise" and last["counts"] is None and last["nan_seq"] is None
    # the segments tile the script and split no NaN pair
    assert E.A_SEGMENTS[0][0] == 0 and E.A_SEGMENTS[-1][1] == len(A)
    assert all(a[1] == b[0] for a, b in zip(E.A_SEGMENTS, E.A_SEGMENTS[1:])) and all(lo < hi for lo, hi in E.A_SEGMENTS)
    assert not any(A[lo]["nan_pair"] for lo, _ in E.A_SEGMENTS)


@pytest.mark.parametrize("name", sorted(E.GRAPH_SCRIPTS))
def test_graph_scripts_fill_and_overflow_the_cache(name):
    script, cap, fields = E.GRAPH_SCRIPTS[name]
    assert all(s["B"] <= cap[0] and s["N"] <= cap[1] and s["B"] * s["N"] <= 1040 for s in script)
    samples = [s for s in script if s["kind"] == "sample"]
    assert len({s["seed"] for s in samples}) == len(samples)                     # a revisit runs on other inputs
    events = E.simulate_cache(script)
    keys = {k for k, _ in events}
    assert len(keys) >= E.PD_GRAPH_CACHE_MAX + 2
    assert {e for _, e in events} == {"capture", "replay", "recapture"}          # a revisit of an evicted key and one of a cached key
    assert all(sum(1 for k2, _ in events if k2 == k) >= 2 for k in keys)         # every key is visited again
    first = [k for k, e in events if e == "capture"]
    again = [k for k, e in events[len(first):]]
    assert again[:len(first)] != first                                           # ... in another order
    for f in fields:
        assert any(E.differ_only_in(a, b, f) for a in keys for b in keys), f
    has_streamed = cap[0] * cap[1] >= E.PD_STREAM_MIN_ROWS
    assert has_streamed or all(s["split"] == 0 for s in script)
    # guided keys come after their scene's upload and fit it
    up = [i for i, s in enumerate(script) if s["kind"] == "matches"]
    for i, s in enumerate(script):
        if s["kind"] == "sample" and s["scene"]:
            sc = E.SCENES[s["scene"]]
            assert any(j < i and script[j]["scene"] == s["scene"] for j in up) and (s["B"], s["N"]) == (sc["B"], sc["N"])
            assert 0 < s["cond_start"] <= (E.B_TIMESTEPS if name == "B" else E.C_TIMESTEPS)


def test_graph_scripts_cover_every_key_field_between_them():
    fields = set()
    for _, _, f in E.GRAPH_SCRIPTS.values():
        fields |= set(f)
    assert fields == set(E.KEY_OPTION_FIELDS)
    assert set(E.C_FIELDS) == set(E.KEY_OPTION_FIELDS)                           # the engine with the streamed path varies all five
    B, C = E.SCRIPT_B, E.SCRIPT_C
    assert any(s["phases"] == "split" and s["scene"] for s in B)
    assert len({(s["B"], s["N"]) for s in B if s["kind"] == "sample"}) >= 4
    paths = {E.path_of(s, E.C_CAP) for s in C if s["kind"] == "sample"}
    assert paths == set(E.PATHS)
    # a second z at an unchanged, still cached key
    samples = [s for s in C if s["kind"] == "sample"]
    ev = E.simulate_cache(C)
    assert all(s["phases"] == "all" for s in samples) and len(ev) == len(samples)          # one key per step
    assert any(e == "replay" and a["seed"] != b["seed"] and E.graph_keys(a) == E.graph_keys(b)
               for a, b, (_, e) in zip(samples, samples[1:], ev[1:]))


def test_script_d_shapes_go_up_and_down():
    D = E.SCRIPT_D
    rows = [s["B"] * s["N"] for s in D]
    assert any(a < b for a, b in zip(rows, rows[1:])) and any(a > b for a, b in zip(rows, rows[1:]))
    assert all(s["B"] <= E.D_CAP[0] and s["N"] <= E.D_CAP[1] and s["split"] == 0 for s in D)
    assert any(a["counts"] and b["counts"] is None and a["kind"] == b["kind"] == "denoise" for a, b in zip(D, D[1:]))
    assert any(a["nan_seq"] is not None and b["nan_pair"] for a, b in zip(D, D[1:]))
    assert len({(s["B"], s["N"]) for s in D if s["kind"] == "sample" and s["counts"] is None}) >= 2
    assert D[-1] == D[0]
    cfgs = E.d_configs()
    assert cfgs[0].d == 32 and not cfgs[1].norm_first and not cfgs[1].pivot
