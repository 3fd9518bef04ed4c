"""Device-side match ingestion with one frame count per sequence (pd_ggs_set_matches_csr_async_nf): what an upload costs.

(a) One sequence of 64 / 96 / 128 / 256 frames x 300 matches per one-order pair (up to 9.8 M matches), inputs resident on the device:
      device   hipEvents around the call (the kernels), and the wall time of the call itself -- which must stay a launch cost;
      host     the wall time of pd_ggs_set_matches (synchronous host sort + copy), whose code this change does not touch.
(b) A ragged call of 32 sequences of 8 .. 20 frames x 300 per pair through the new export, against the runs of equal-count slots it
    replaces through pd_ggs_set_matches_csr_async (one call per run of consecutive equal counts; the sequences sorted by count so that
    the runs are as long as they can be).
One process, variants in alternation, ROUNDS rounds; a figure is the median of its rounds, the spread (max - min) / median.  Synthetic
matches (uniform points; the sort does not look at them), rows shuffled.
(c) `one256`: nothing but WARM + 3 uploads of the 256-frame sequence -- the process to run under a kernel tracer for per-kernel times.

usage: python tests/perf/ingest_long_bench.py [out.txt | one256]      (default out: profiles/ingest_long_frames.txt)"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from posediffusion_amd import synth                                     # noqa: E402
from posediffusion_amd.engine import PoseEngine                         # noqa: E402
from posediffusion_amd.host import denoiser_state, pack_matches, pack_matches_ragged   # noqa: E402

DEV = torch.device("cuda:0")
PER_PAIR, IMG, ROUNDS, WARM = 300, 224, 7, 2


def matches(N, seed):
    rng = np.random.default_rng(seed)
    pairs = np.array([(i, j) for i in range(N) for j in range(i + 1, N)], dtype=np.int64)
    i12 = np.repeat(pairs, PER_PAIR, 0)[rng.permutation(len(pairs) * PER_PAIR)]
    M = len(i12)
    return {"kp1": rng.uniform(0, IMG, (M, 2)), "kp2": rng.uniform(0, IMG, (M, 2)), "i12": i12, "img_shape": (N, 3, IMG, IMG)}


def med(v):
    return statistics.median(v), (max(v) - min(v)) / statistics.median(v)


def timed_device(fn):
    """(device ms between two events around fn, wall ms of fn itself)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    fn()
    wall = (time.perf_counter() - t0) * 1e3
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), wall


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ingest_long_frames.txt")
    diff = synth.make_diffuser(seed=0).to(DEV)
    tables = {k: v for k, v in diff.named_buffers(recurse=False)}
    eng = PoseEngine(denoiser_state(diff.model), tables, device=DEV, max_B=32, max_N=256, ggs_max_frames=256)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    frames = (256,) if out_path == "one256" else (64, 96, 128, 256)
    say(f"(a) one sequence, {PER_PAIR} matches per one-order pair, device-resident inputs; median of {ROUNDS} rounds (spread)")
    say("frames    matches   device upload: kernels ms   call wall ms   | host upload (pd_ggs_set_matches) wall ms")
    for N in frames:
        md = matches(N, N)
        kp1, kp2, i12, off, shape, counts = pack_matches_ragged([md], pin=False)
        kp1, kp2, i12 = kp1.to(DEV), kp2.to(DEV), i12.to(DEV)
        hints = dict(max_pairs=N * (N - 1) // 2, max_matches_per_pair=PER_PAIR, one_order=True)
        dev_ms, wall_ms, host_ms = [], [], []
        for r in range(WARM + (3 if out_path == "one256" else ROUNDS)):
            d, w = timed_device(lambda: eng.set_matches_async(0, kp1, kp2, i12, off, shape, n_frames=counts, **hints))
            eng.check_async()
            if out_path != "one256":
                t0 = time.perf_counter()
                eng.set_matches(1, md["kp1"], md["kp2"], md["i12"], md["img_shape"])
                h = (time.perf_counter() - t0) * 1e3
            else:
                h = 0.0
            if r >= WARM:
                dev_ms.append(d)
                wall_ms.append(w)
                host_ms.append(h)
        (d, ds), (w, ws), (h, hs) = med(dev_ms), med(wall_ms), med(host_ms) if host_ms[0] else (0.0, 0.0)
        say(f"{N:6d} {len(md['kp1']):10d}   {d:10.2f} ({ds:4.0%})   {w:8.2f} ({ws:4.0%})   | {h:10.1f} ({hs:4.0%})")
    if out_path == "one256":
        return
    counts32 = sorted(int(v) for v in np.random.default_rng(5).integers(8, 21, 32))
    mds = [matches(n, 100 + b) for b, n in enumerate(counts32)]
    runs, a = [], 0
    for b in range(1, 33):
        if b == 32 or counts32[b] != counts32[a]:
            runs.append((a, b))
            a = b
    ragged = [t.to(DEV) if isinstance(t, torch.Tensor) else t for t in pack_matches_ragged(mds, pin=False)]
    grouped = [(a, [t.to(DEV) if isinstance(t, torch.Tensor) else t for t in pack_matches(mds[a:b], pin=False)]) for a, b in runs]

    def one_call():
        eng.set_matches_async(0, *ragged[:5], n_frames=ragged[5], max_matches_per_pair=PER_PAIR)

    def equal_count_runs():
        for a, packed in grouped:
            eng.set_matches_async(a, *packed, max_matches_per_pair=PER_PAIR)

    res = {"ragged": ([], []), "runs": ([], [])}
    for r in range(WARM + ROUNDS):
        for name, fn in (("ragged", one_call), ("runs", equal_count_runs)):
            d, w = timed_device(fn)
            eng.check_async()
            if r >= WARM:
                res[name][0].append(d)
                res[name][1].append(w)
    say(f"(b) 32 sequences of {counts32[0]} .. {counts32[-1]} frames ({len(runs)} distinct counts), {sum(len(m['kp1']) for m in mds)} matches")
    for name, label in (("ragged", "one call with n_frames (new export)"), ("runs", f"{len(runs)} calls of equal-count slots (old export)")):
        (d, ds), (w, ws) = med(res[name][0]), med(res[name][1])
        say(f"  {label:48s} kernels {d:7.3f} ms ({ds:4.0%})   calls' wall {w:7.3f} ms ({ws:4.0%})")
    eng.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
