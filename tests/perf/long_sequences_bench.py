"""One denoiser step (pd_time_kernel, what = 0: the launches of a sampling step, z piece prepared outside) at sequences of 128 and 256 frames
against the existing 64-frame shapes with the SAME number of token rows, which the parent commit can run as well:

    1 024 rows: (16, 64)  (8, 128)  (4, 256)          5 120 rows: (80, 64)  (40, 128)  (20, 256)

At equal rows every GEMM, LayerNorm and the tail do the same work; only attention differs -- its score and P V work per row doubles with N,
and above 64 frames it runs the key-tiled pd_attn_long_kernel (csrc/pd_attn_long.h) in place of pd_attn_seq_kernel.  The 64-frame shapes
are also timed with the tiled kernel forced (PD_OPT_DENOISER_LONG_ATTN = 1): the same work on the other kernel.

One process, one box: all variants are timed in alternation, ROUNDS rounds of REPS steps each; the figure of a variant is the median of
its rounds, the spread its (max - min) / median.  Modes: the engine's default (fp16 planes) and exact fp32 (PD_OPT_DENOISER_SPLIT = 0).
usage: python tests/perf/long_sequences_bench.py [out.txt]  -> the table (also written to out.txt, default profiles/long_sequences.txt) + one JSON line"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from posediffusion_amd import _lib, synth                     # noqa: E402
from posediffusion_amd.engine import PoseEngine               # noqa: E402
from posediffusion_amd.host import denoiser_state             # noqa: E402

DEV = torch.device("cuda:0")
GROUPS = {1024: [(16, 64), (8, 128), (4, 256)], 5120: [(80, 64), (40, 128), (20, 256)]}
ROUNDS, REPS = 11, 20


def main():
    if not torch.cuda.is_available():
        raise RuntimeError("long_sequences_bench.py measures on an AMD GPU; none is visible")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "long_sequences.txt")
    diff = synth.make_diffuser(seed=0)
    synth.randomize_norm_and_bias_(diff.model)
    diff = diff.to(DEV)
    eng = PoseEngine(denoiser_state(diff.model), {k: v for k, v in diff.named_buffers(recurse=False)}, device=DEV, max_B=80, max_N=256)
    # pd_time_kernel reads the sampler's buffers: fill them with one unguided sampling call at the engine's capacity
    z = synth.make_z(80, 256).to(DEV)
    noise = torch.randn(101, 80, 256, 9, generator=torch.Generator(device=DEV).manual_seed(0), device=DEV)
    pose, _, _ = eng.sample(z, noise, 0, None, use_graph=False, want_process=False)
    assert torch.isfinite(pose).all()
    variants = []                                             # (rows, B, N, split mode, forced tiled kernel)
    for rows, shapes in GROUPS.items():
        for mode in (2, 0):
            for B, N in shapes:
                variants.append((rows, B, N, mode, 0))
                if N == 64:
                    variants.append((rows, B, N, mode, 1))

    def run(v, reps):
        _, B, N, mode, forced = v
        eng.set_split_precision(mode)
        eng.set_option(_lib.PD_OPT_DENOISER_LONG_ATTN, forced)
        return eng.time_kernel(0, B, N, reps=reps) * 1e3      # us per step

    for v in variants:
        run(v, 3)
    times = {v: [] for v in variants}
    for _ in range(ROUNDS):
        for v in variants:
            times[v].append(run(v, REPS))
    eng.set_option(_lib.PD_OPT_DENOISER_LONG_ATTN, 0)
    eng.set_split_precision(2)
    med = {v: statistics.median(t) for v, t in times.items()}
    lines = [f"one denoiser step (pd_time_kernel what = 0), {ROUNDS} interleaved rounds of {REPS} steps, median us per step "
             "(spread = (max - min) / median); ratio = against the 64-frame shape of the same rows and mode"]
    ratios = {}
    for rows, shapes in GROUPS.items():
        for mode in (2, 0):
            base = med[(rows, shapes[0][0], 64, mode, 0)]
            lines.append(f"{rows} token rows, PD_OPT_DENOISER_SPLIT = {mode}")
            for v in variants:
                if v[0] != rows or v[3] != mode:
                    continue
                _, B, N, _, forced = v
                name = f"({B}, {N})" + (" tiled kernel forced" if forced else "")
                lines.append(f"  {name:32s} {med[v]:9.1f} us   spread {(max(times[v]) - min(times[v])) / med[v]:.2f}   ratio {med[v] / base:.3f}")
                ratios[f"{rows}_split{mode}_b{B}n{N}" + ("_forced" if forced else "")] = round(med[v] / base, 3)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    print(json.dumps({"us": {f"{v[0]}_split{v[3]}_b{v[1]}n{v[2]}" + ("_forced" if v[4] else ""): round(m, 1) for v, m in med.items()}, "ratio": ratios}))
    eng.close()


if __name__ == "__main__":
    main()
