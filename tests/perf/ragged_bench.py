"""Sequences of different frame counts in one padded batch (pd_engine_set_frame_counts): what it costs and what it buys.

(a) The uniform path must not have moved.  pd_time_kernel (what = 0: one denoiser step, what = 1: one pd_ggs_guide) at the bench shapes
    (64 and 256 sequences of 20 frames) on THIS build and on the PARENT commit's library, both loaded into this one process (the parent's
    with RTLD_LOCAL | RTLD_DEEPBIND, before this build's), each with its own engine holding the same weights, inputs and matches; timed in
    alternation.  The claim to check: this build sits inside the spread of the parent's own rounds.
(b) One guided sampling pass (cond_start_step = 10, hipGraph replay) of 256 sequences with frame counts drawn from 8 .. 20:
      ragged   one padded call [256, 20, .] with the counts set;
      grouped  the same sequences as 13 uniform calls, one per frame count, issued back to back on one stream (what a service does
               today: one engine per count, each call a small launch);
      uniform  256 sequences of 20 frames in one uniform call -- against `ragged` the price of the padding rows the ragged call carries.
    Matches are epipolar-consistent with each sequence's own model mean where guidance starts (bench_legs.make_batch_inputs' recipe), so
    every guided step runs its full 700 iterations.

One process, one box: all variants in alternation, ROUNDS rounds; the figure of a variant is the median of its rounds, the spread its
(max - min) / median.
usage: python tests/perf/ragged_bench.py [out.txt] [parent libpd_engine.so] [a_only]   (default out: profiles/ragged_batches.txt; without a
parent library part (a) reports this build alone and says so; a_only: part (a) alone -- with a COPY of this build's library as the "parent"
that is the A / A control of the two-libraries-in-one-process method itself)"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from posediffusion_amd import _lib, synth                     # noqa: E402
from posediffusion_amd.engine import PoseEngine, make_ggs_cfg  # noqa: E402
from posediffusion_amd.host import denoiser_state, draw_noise  # noqa: E402

DEV = torch.device("cuda:0")
N_MAX, B_ALL, COND_START, PER_PAIR, IMG = 20, 256, 10, 300, 224
ROUNDS_A, REPS_DEN, REPS_GGS, ROUNDS_B = 9, 20, 2, 7


def load_parent(path):
    """The parent commit's build beside this one: its own symbols first (DEEPBIND), none of them visible to anybody else (LOCAL)."""
    lib = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def engine_on(lib, diff, max_B, max_N):
    cur = _lib._lib
    _lib._lib = lib
    try:
        return PoseEngine(denoiser_state(diff.model), {k: v for k, v in diff.named_buffers(recurse=False)}, device=DEV, max_B=max_B, max_N=max_N)
    finally:
        _lib._lib = cur


def guided_inputs(eng, counts, seed0):
    """z, reference-order noise and per-sequence matches consistent with the sequence's own model mean at t = COND_START - 1 (padded batch;
    counts None: uniform N_MAX frames)."""
    B = len(counts)
    z = torch.cat([synth.make_z(1, N_MAX, seed=1000 + seed0 + b) for b in range(B)]).to(DEV)
    noise = draw_noise((B, N_MAX, 9), 100, DEV, COND_START, True, generator=torch.Generator(device=DEV).manual_seed(seed0))
    nf = None if all(n == N_MAX for n in counts) else counts
    _, process, _ = eng.sample(z, noise, 0, None, use_graph=False, n_frames=nf)
    mean, _ = eng.p_mean(process[100 - COND_START], z, COND_START - 1, n_frames=nf)
    mean = mean.cpu().numpy().astype(np.float64)
    mds = [synth.make_epipolar_matches(mean[b, :n], IMG, IMG, PER_PAIR, seed=2000 + seed0 + b) for b, n in enumerate(counts)]
    return z, noise, mds


def upload(eng, mds, slots=None):
    for s, md in enumerate(mds):
        eng.set_matches(s if slots is None else slots[s], md["kp1"], md["kp2"], md["i12"], md["img_shape"])


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def med_spread(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m


def family(eng, B, N, cfg, nf=None):
    p = eng.ggs_plan(B, N, cfg, n_frames=nf)
    return "lane" if p[6] else (f"two_hop_k{p[0]}" if p[3] else (f"one_hop_k{p[0]}" if p[0] > 1 else f"wave_k1_{p[4]}w"))


def main():
    if not torch.cuda.is_available():
        raise RuntimeError("ragged_bench.py measures on an AMD GPU; none is visible")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ragged_batches.txt")
    parent_path = sys.argv[2] if len(sys.argv) > 2 else None
    parent = load_parent(parent_path) if parent_path else None       # before this build is loaded (RTLD_GLOBAL)
    this = _lib.load()
    diff = synth.make_diffuser(seed=0)
    synth.randomize_norm_and_bias_(diff.model)
    diff = diff.to(DEV)
    cfg = make_ggs_cfg(synth.GGS_CFG)
    lines, js = [], {}

    # ---------------------------------------------------------------- (a) the uniform path, this build against the parent's
    eng = engine_on(this, diff, B_ALL, N_MAX)
    uni = (N_MAX,) * B_ALL
    z_u, noise_u, mds_u = guided_inputs(eng, uni, 0)
    upload(eng, mds_u)
    builds = {"this": eng}
    if parent is not None:
        builds["parent"] = engine_on(parent, diff, B_ALL, N_MAX)
        upload(builds["parent"], mds_u)
    for e in builds.values():                                         # pd_time_kernel reads the sampler's buffers: one guided pass fills them
        pose, _, _ = e.sample(z_u, noise_u, COND_START, cfg, use_graph=False, want_process=False)
        e.check_async()
        assert torch.isfinite(pose).all()
    variants = [(what, B, name) for what in (0, 1) for B in (64, B_ALL) for name in builds]
    run_a = lambda v, reps: builds[v[2]].time_kernel(v[0], v[1], N_MAX, cfg, reps=reps) * 1e3     # noqa: E731  (us per launch)
    for v in variants:
        run_a(v, 2)
    times = {v: [] for v in variants}
    for _ in range(ROUNDS_A):
        for v in variants:
            times[v].append(run_a(v, REPS_GGS if v[0] else REPS_DEN))
    lines.append(f"(a) uniform path, pd_time_kernel at N = {N_MAX}: {ROUNDS_A} interleaved rounds ({REPS_DEN} denoiser steps / {REPS_GGS} GGS launches each), "
                 "median us per launch, spread = (max - min) / median, [min .. max]" + ("" if parent is not None else "   (no parent library given: this build alone)"))
    for what in (0, 1):
        for B in (64, B_ALL):
            row = f"  {'denoiser step' if what == 0 else 'pd_ggs_guide ':14s} B = {B:3d} ({family(eng, B, N_MAX, cfg) if what else 'fp16 planes'}):"
            for name in builds:
                t = times[(what, B, name)]
                m, s = med_spread(t)
                row += f"   {name} {m:10.1f} us  spread {s:.3f} [{min(t):.1f} .. {max(t):.1f}]"
                js[f"a_{'den' if what == 0 else 'ggs'}_b{B}_{name}_us"] = round(m, 1)
            if parent is not None:
                tp, tt = times[(what, B, "parent")], statistics.median(times[(what, B, "this")])
                row += f"   this / parent {tt / statistics.median(tp):.4f}   inside the parent's rounds: {min(tp) <= tt <= max(tp)}"
            lines.append(row)
    if parent is not None:
        builds["parent"].close()
    if len(sys.argv) > 3 and sys.argv[3] == "a_only":
        text = "\n".join(lines) + "\n"
        print(text, end="")
        with open(out_path, "w") as fh:
            fh.write(text)
        print(json.dumps(js))
        return

    # ---------------------------------------------------------------- (b) one guided sampling pass of 256 sequences, counts 8 .. 20
    rng = np.random.default_rng(11)
    counts = tuple(int(v) for v in rng.integers(8, N_MAX + 1, B_ALL))
    z_r, noise_r, mds_r = guided_inputs(eng, counts, 5000)
    eng_u = eng                                                        # holds the 20-frame matches of (a)
    eng_r = engine_on(this, diff, B_ALL, N_MAX)
    upload(eng_r, mds_r)
    groups = {}
    for n in sorted(set(counts)):
        idx = [b for b, c in enumerate(counts) if c == n]
        ge = engine_on(this, diff, len(idx), n)
        upload(ge, [mds_r[b] for b in idx])
        it = torch.as_tensor(idx, device=DEV)
        groups[n] = (ge, z_r[it, :n].contiguous(), noise_r[:, it, :n].contiguous(), idx)
    fam_r = family(eng_r, B_ALL, N_MAX, cfg, counts)
    fam_g = {n: family(g[0], len(g[3]), n, cfg) for n, g in groups.items()}

    def run_ragged():
        return eng_r.sample(z_r, noise_r, COND_START, cfg, use_graph=True, want_process=False, n_frames=counts)

    def run_grouped():
        return [g[0].sample(g[1], g[2], COND_START, cfg, use_graph=True, want_process=False) for g in groups.values()]

    def run_uniform():
        return eng_u.sample(z_u, noise_u, COND_START, cfg, use_graph=True, want_process=False)

    runs = {"ragged": run_ragged, "grouped": run_grouped, "uniform": run_uniform}
    res = {k: f() for k, f in runs.items()}                            # warm: graphs captured
    torch.cuda.synchronize()
    for e in [eng_r, eng_u] + [g[0] for g in groups.values()]:
        e.check_async()
    pose_r, _, st_r = res["ragged"]
    full = int((st_r[:, :, :, 1].sum(dim=2) == 700).sum()), st_r.shape[0] * st_r.shape[1]
    worst = 0.0                                                        # the ragged slots against the same sequences in their uniform groups
    for (ge, _, _, idx), (pg, _, _) in zip(groups.values(), res["grouped"]):
        n = pg.shape[1]
        worst = max(worst, float(((pose_r[idx, :n] - pg).abs().max() / pg.abs().max()).item()))
    assert torch.isfinite(pose_r).all()
    tb = {k: [] for k in runs}
    for _ in range(ROUNDS_B):
        for k, f in runs.items():
            tb[k].append(timed(f))
    frames = sum(counts)
    lines.append(f"(b) one guided sampling pass (100 steps, the last {COND_START} guided x 700 iterations, hipGraph replay) of {B_ALL} sequences, "
                 f"frame counts uniform in 8 .. {N_MAX} ({frames} frames, {B_ALL * N_MAX - frames} padding rows = {1 - frames / (B_ALL * N_MAX):.1%} of the padded batch), "
                 f"{PER_PAIR} matches per pair; {ROUNDS_B} interleaved rounds, median ms per pass")
    lines.append(f"  attention kernel of the ragged pass: pd_attn_long_kernel<2> (key-tiled, a length per sequence; fp16-plane path, 5 120 token rows); "
                 f"GGS: {fam_r}; guided (step, sequence) pairs that ran all 700 iterations: {full[0]} of {full[1]}")
    lines.append(f"  grouped: {len(groups)} uniform calls of {[len(g[3]) for g in groups.values()]} sequences at N = {list(groups)} on the small-batch path; GGS {sorted(set(fam_g.values()))}")
    lines.append(f"  ragged slots against the same sequences in their uniform groups (other denoiser path, other GGS family: rounding-level inputs "
                 f"amplified by 7 000 iterations): worst max|d| / max|pose| = {worst:.2e}")
    m = {k: med_spread(v) for k, v in tb.items()}
    for k in runs:
        lines.append(f"  {k:8s} {m[k][0]:9.2f} ms  spread {m[k][1]:.3f}   {B_ALL / m[k][0] * 1e3:8.1f} sequences / s")
        js[f"b_{k}_ms"] = round(m[k][0], 2)
    lines.append(f"  ragged / grouped {m['ragged'][0] / m['grouped'][0]:.3f}   ragged / uniform-20 {m['ragged'][0] / m['uniform'][0]:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    print(json.dumps(js))


if __name__ == "__main__":
    main()
