"""GGS above 64 frames (PD_OPT_GGS_MAX_FRAMES, pd_ggs_long_kernel): what an iteration costs, and that launches at N <= 64 did not move.

  1. us per GGS iteration at B = 1, exhaustive one-order pairs with 300 matches each, at 64 frames (two-hop kernel), 64 (long kernel forced,
     PD_GGS_CFG_LONG_FRAMES), 96, 128 and 256 frames (157 MB of matches).  One process, ROUNDS interleaved rounds; an iteration's cost is the
     difference of two GGS_optimize launches of 2 x I_LONG and 2 x I_SHORT iterations (min_matches = 0: no early exit), which takes the launch,
     the zeroing of the exchange region and the table loads out.
  2. The in-kernel phase clocks (pd_debug_ggs_prof) of workgroup 0 and of the last workgroup at 128 frames.
  3. pd_time_kernel(what = 1) at (B, N) = (256, 20) and (1, 50) with this library and, where --parent-lib names one, the parent commit's,
     in alternating fresh child processes (each under its own time limit); the spread of each library's own repeats stands next to the
     difference.

usage: python tests/perf/ggs_long_bench.py [--parent-lib libpd_engine.so] [out.txt]   (default profiles/ggs_long_frames.txt)"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from posediffusion_amd import _lib, synth                     # noqa: E402
from posediffusion_amd.engine import PoseEngine, make_ggs_cfg  # noqa: E402
from posediffusion_amd.host import denoiser_state             # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS, I_SHORT, I_LONG = 7, 5, 30
PER_PAIR = 300
AB_SHAPES = ((256, 20), (1, 50))
AB_ROUNDS, AB_REPS, AB_ITER = 2, 5, 20
CHILD_LIMIT_S = 240


def _engine(max_B, max_N, **kw):
    diff = synth.make_diffuser(seed=0)
    synth.randomize_norm_and_bias_(diff.model)
    diff = diff.to(DEV)
    return PoseEngine(denoiser_state(diff.model), {k: v for k, v in diff.named_buffers(recurse=False)}, device=DEV, max_B=max_B, max_N=max_N, **kw)


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3      # us


def iteration_table(lines):
    eng = _engine(1, 256, ggs_max_frames=256)
    variants = [(64, 0), (64, _lib.PD_GGS_CFG_LONG_FRAMES), (96, 0), (128, 0), (256, 0)]
    scenes, plans = {}, {}
    for N in sorted({n for n, _ in variants}):
        enc = synth.make_cameras(N, seed=800 + N)
        scenes[N] = (synth.make_matches(enc, 224, 224, per_pair=PER_PAIR, seed=800 + N), synth.perturb_pose(enc, seed=810 + N).to(DEV))
    times = {v: [] for v in variants}
    cur = None

    def run(v, iters):
        nonlocal cur
        N, flag = v
        md, x = scenes[N]
        if cur != N:
            eng.set_matches(0, md["kp1"], md["kp2"], md["i12"], md["img_shape"])
            cur = N
        cfg = make_ggs_cfg(iter_num=iters, min_matches=0, reserved=flag)
        plans[v] = eng.ggs_plan(1, N, cfg)
        return _timed(lambda: eng.ggs_optimize(x, cfg=cfg))

    for r in range(ROUNDS + 1):                                # round 0 warms up
        for v in variants:
            t_short, t_long = run(v, I_SHORT), run(v, I_LONG)
            if r:
                times[v].append((t_long - t_short) / (2 * (I_LONG - I_SHORT)))
    eng.check_async()
    lines.append(f"us per GGS iteration, B = 1, all one-order pairs x {PER_PAIR} matches; {ROUNDS} interleaved rounds, median "
                 f"(spread = (max - min) / median); plan = [k, slots, LDS bytes, kernel (1 two-hop, 2 long), ...]")
    res = {}
    for v in variants:
        N, flag = v
        med = statistics.median(times[v])
        name = f"{N} frames" + (" (long kernel forced)" if flag else "")
        lines.append(f"  {name:32s} {N * (N - 1) // 2:6d} pairs  {med:9.2f} us   spread {(max(times[v]) - min(times[v])) / med:.2f}   plan {plans[v][:4]}")
        res[f"n{N}" + ("_forced" if flag else "")] = round(med, 2)
    # phase clocks at 128 frames: counters [0..7] workgroup 0, [8..15] the last workgroup
    md, x = scenes[128]
    eng.set_matches(0, md["kp1"], md["kp2"], md["i12"], md["img_shape"])
    buf = (C.c_longlong * 16)()
    _lib.check(eng.lib.pd_debug_ggs_prof(eng._h, 1, None), "pd_debug_ggs_prof")
    iters = 2 * I_LONG
    eng.ggs_optimize(x, cfg=make_ggs_cfg(iter_num=I_LONG, min_matches=0))
    _lib.check(eng.lib.pd_debug_ggs_prof(eng._h, 0, buf), "pd_debug_ggs_prof")
    names = ["P1", "P2", "P3a", "hop-1 publish + totals", "P3b owner loop", "hop-2 gathers", "frame gradients + totals", "P4"]
    lines.append(f"phase clocks at 128 frames (pd_debug_ggs_prof), clock ticks per iteration over {iters} iterations: workgroup 0 | last workgroup")
    for i, n in enumerate(names):
        lines.append(f"  {n:26s} {buf[i] / iters:10.1f} | {buf[8 + i] / iters:10.1f}")
    res["prof128_wg0"] = [round(buf[i] / iters, 1) for i in range(8)]
    eng.close()
    return res


def child_ab():
    """one fresh process: pd_time_kernel(what = 1) at the A / B shapes with the library PD_ENGINE_LIB names (or the tree's)"""
    out = {}
    for B, N in AB_SHAPES:
        eng = _engine(B, N)
        enc = synth.make_cameras(N, seed=800 + N)
        md = synth.make_matches(enc, 224, 224, per_pair=PER_PAIR, seed=800 + N)
        for b in range(B):
            eng.set_matches(b, md["kp1"], md["kp2"], md["i12"], md["img_shape"])
        z = synth.make_z(B, N).to(DEV)
        noise = torch.randn(101, B, N, 9, generator=torch.Generator(device=DEV).manual_seed(0), device=DEV)
        eng.sample(z, noise, 0, None, use_graph=False, want_process=False)        # fills the buffers pd_time_kernel reads
        cfg = make_ggs_cfg(dict(synth.GGS_CFG, iter_num=AB_ITER, min_matches=0))
        eng.time_kernel(1, B, N, cfg, reps=2)
        out[f"b{B}n{N}"] = [round(eng.time_kernel(1, B, N, cfg, reps=AB_REPS), 4) for _ in range(3)]
        eng.close()
    print("AB " + json.dumps(out))


def ab_table(lines, parent_lib):
    libs = {"this": None, "parent": parent_lib}
    runs = {k: {f"b{B}n{N}": [] for B, N in AB_SHAPES} for k in libs}
    for _ in range(AB_ROUNDS):
        for name, path in libs.items():
            env = dict(os.environ)
            env.pop("PD_ENGINE_LIB", None)
            if path:
                env["PD_ENGINE_LIB"] = path
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-ab"], env=env, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
            if p.returncode != 0:
                raise RuntimeError(f"A / B child ({name}) ended with {p.returncode}: {p.stderr[-800:]}")
            got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("AB ")][-1][3:])
            for k, v in got.items():
                runs[name][k] += v
    lines.append(f"pd_time_kernel(what = 1), iter_num = {AB_ITER}, ms per launch: {AB_ROUNDS} alternating fresh processes per library x 3 repeats of "
                 f"{AB_REPS} launches; median (spread = (max - min) / median)")
    res = {}
    for B, N in AB_SHAPES:
        k = f"b{B}n{N}"
        m = {n: statistics.median(runs[n][k]) for n in libs}
        s = {n: (max(runs[n][k]) - min(runs[n][k])) / m[n] for n in libs}
        lines.append(f"  ({B}, {N}): this {m['this']:.4f} ms (spread {s['this']:.3f})   parent {m['parent']:.4f} ms (spread {s['parent']:.3f})   "
                     f"this / parent {m['this'] / m['parent']:.4f}")
        res[k] = {"this": m["this"], "parent": m["parent"], "spread": max(s.values())}
    return res


def main():
    if not torch.cuda.is_available():
        raise RuntimeError("ggs_long_bench.py measures on an AMD GPU; none is visible")
    args = sys.argv[1:]
    if args and args[0] == "--child-ab":
        return child_ab()
    parent_lib = None
    if args and args[0] == "--parent-lib":
        parent_lib, args = os.path.abspath(args[1]), args[2:]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "ggs_long_frames.txt")
    lines, res = [], {}
    res["iteration_us"] = iteration_table(lines)
    if parent_lib:
        res["ab"] = ab_table(lines, parent_lib)
    else:
        lines.append("pd_time_kernel A / B against the parent commit's library: not run (no --parent-lib)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
