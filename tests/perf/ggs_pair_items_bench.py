"""GGS above 64 frames with frame pairs of several work items (PD_OPT_GGS_LONG_PAIR_ITEMS, pd_ggs_longm_kernel): what the slot-is-a-pair form
costs where it is not needed, and what serialising a pair's items on one wave costs where it is.

96 frames, B = 1, all 4 560 one-order pairs; one process, one engine per variant (no re-upload between rounds), ROUNDS interleaved rounds
after a warm-up round.  An iteration's cost is the difference of two GGS_optimize launches of 60 and 10 iterations (iter_num = 30 and 5,
all three groups: x 2; min_matches = 0: no early exit) divided by 50, which takes the launch, the zeroing of the exchange region and the
table loads out.

  (a) 300 matches per pair on pd_ggs_long_kernel (host-built tables) and on pd_ggs_longm_kernel (the same data through device-side
      ingestion with max_matches_per_pair = 0, whose host shadow is not one item per pair; the pair hints are exact, so both launches have
      the same workgroups and slots and differ in the kernel alone).
  (b) 1 000 and 2 000 matches per pair (2 and 4 work items) on pd_ggs_longm_kernel, next to (a) scaled by the matches.

usage: python tests/perf/ggs_pair_items_bench.py [out.txt]   (default profiles/ggs_long_pair_items.txt)"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from posediffusion_amd import synth                            # noqa: E402
from posediffusion_amd.engine import PoseEngine, make_ggs_cfg  # noqa: E402
from posediffusion_amd.host import denoiser_state, pack_matches_ragged   # noqa: E402

DEV = torch.device("cuda:0")
N = 96
ROUNDS, I_SHORT, I_LONG = 7, 5, 30
VARIANTS = (("a_long_300", 300, "host", 2), ("a_pair_300", 300, "device", 3), ("b_pair_1000", 1000, "host", 3), ("b_pair_2000", 2000, "host", 3))


def _engine():
    diff = synth.make_diffuser(seed=0)
    synth.randomize_norm_and_bias_(diff.model)
    diff = diff.to(DEV)
    return PoseEngine(denoiser_state(diff.model), {k: v for k, v in diff.named_buffers(recurse=False)}, device=DEV, max_B=1, max_N=N,
                      ggs_max_frames=N, ggs_long_pair_items=True)


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3      # us


def main():
    if not torch.cuda.is_available():
        raise RuntimeError("ggs_pair_items_bench.py measures on an AMD GPU; none is visible")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ggs_long_pair_items.txt")
    enc = synth.make_cameras(N, seed=800 + N)
    x = synth.perturb_pose(enc, seed=810 + N).to(DEV)
    scenes, engines, plans = {}, {}, {}
    for name, per_pair, how, kernel in VARIANTS:
        if per_pair not in scenes:
            scenes[per_pair] = synth.make_matches(enc, 224, 224, per_pair=per_pair, seed=800 + N)
        md = scenes[per_pair]
        e = engines[name] = _engine()
        if how == "host":
            e.set_matches(0, md["kp1"], md["kp2"], md["i12"], md["img_shape"])
        else:
            kp1, kp2, i12, off, shape, counts = pack_matches_ragged([md], pin=True)
            e.set_matches_async(0, kp1, kp2, i12, off, shape, n_frames=counts, max_pairs=N * (N - 1) // 2, one_order=True, max_matches_per_pair=0)
        plans[name] = e.ggs_plan(1, N, make_ggs_cfg())
        assert plans[name][3] == kernel, (name, plans[name])
        print(f"{name}: {len(md['kp1'])} matches, plan {plans[name]}", flush=True)
    times = {name: [] for name, *_ in VARIANTS}
    for r in range(ROUNDS + 1):                                # round 0 warms up
        for name, *_ in VARIANTS:
            e = engines[name]
            t = [_timed(lambda: e.ggs_optimize(x, cfg=make_ggs_cfg(iter_num=i, min_matches=0))) for i in (I_SHORT, I_LONG)]
            if r:
                times[name].append((t[1] - t[0]) / (2 * (I_LONG - I_SHORT)))
        print(f"round {r} done", flush=True)
    for e in engines.values():
        e.check_async()
        e.close()
    med = {n: statistics.median(v) for n, v in times.items()}
    spread = {n: (max(v) - min(v)) / med[n] for n, v in times.items()}
    pairs = N * (N - 1) // 2
    lines = [f"us per GGS iteration at {N} frames, B = 1, all {pairs} one-order pairs; {ROUNDS} interleaved rounds after a warm-up, median "
             f"(spread = (max - min) / median); an iteration = (launch of {2 * I_LONG} - launch of {2 * I_SHORT} iterations) / {2 * (I_LONG - I_SHORT)}; "
             "plan = [k, slots, LDS bytes, kernel (2 pd_ggs_long_kernel, 3 pd_ggs_longm_kernel), ...]"]
    for name, per_pair, how, _ in VARIANTS:
        scaled = f"   (a) on the same kernel x {per_pair} / 300 = {med['a_pair_300'] * per_pair / 300:9.2f} us" if name.startswith("b_") else ""
        lines.append(f"  {name:12s} {per_pair:5d} matches per pair ({-(-per_pair // 512)} item{'s' if per_pair > 512 else ''}), {how:6s} tables  "
                     f"{med[name]:9.2f} us   spread {spread[name]:.3f}   plan {plans[name][:4]}{scaled}")
    d = med["a_pair_300"] - med["a_long_300"]
    lines.append(f"  (a) pd_ggs_longm_kernel - pd_ggs_long_kernel on single-item pairs: {d:+.2f} us ({d / med['a_long_300']:+.3f} of the long kernel's "
                 f"iteration; the two spreads are {spread['a_long_300']:.3f} and {spread['a_pair_300']:.3f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    print(json.dumps({"us": {n: round(v, 2) for n, v in med.items()}, "spread": {n: round(v, 3) for n, v in spread.items()}}))


if __name__ == "__main__":
    main()
