"""One training step's forward + backward on the trainer for a batch of sequences of DIFFERENT frame counts (pd_trainer_set_frame_counts),
default Denoiser, 8 sequences padded to 64 frames with the counts (64, 50, 40, 33, 20, 10, 5, 3) -- 225 real frames in 512 token rows:

  ragged    one forward + backward at (8, 64) with the counts (the key-tiled attention serves every N while counts are set);
  uniform   the same call without counts (all 512 rows real; the short attention kernels) -- the call that must not get slower;
  loop      what the counts replace: one forward + backward per sequence at (1, n), every parameter gradient computed 8 times (their sum,
            which an optimiser needs, is not even formed here).

The method of tests/perf/train_step_bench.py: one process, the sides run in alternation after warm-up, ROUNDS rounds of REPS steps each,
timed with events on the stream; the figure of a side is the median of its rounds, the spread its (max - min) / median.  Recorded, not
gated.  ``--uniform-only`` times the uniform side alone: with PD_ENGINE_LIB set to another build of the library it is that build's figure
(alternate the two processes to compare builds on one machine).
usage: python tests/perf/train_ragged_bench.py [--uniform-only] [out.txt]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from posediffusion_amd import synth                            # noqa: E402
from posediffusion_amd.host import get_trainer                 # noqa: E402

DEV = torch.device("cuda:0")
B, N = 8, 64
COUNTS = (64, 50, 40, 33, 20, 10, 5, 3)
ROUNDS, REPS, WARMUP = 7, 20, 3


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main(argv):
    uniform_only = "--uniform-only" in argv
    argv = [a for a in argv if a != "--uniform-only"]
    diff = synth.make_diffuser(seed=0)
    synth.randomize_norm_and_bias_(diff.model)
    diff = diff.to(DEV)
    den = diff.model
    sd = {k: p.detach() for k, p in den.named_parameters()}
    g = torch.Generator().manual_seed(B)
    x0, noise = torch.randn(B, N, 9, generator=g).to(DEV), torch.randn(B, N, 9, generator=g).to(DEV)
    z, t = torch.randn(B, N, 384, generator=g).to(DEV), torch.randint(0, 100, (B,), generator=g).to(DEV)
    tr = get_trainer(den, diff, B, N)
    g_loss = torch.full((B, N, 9), 1.0 / (9 * sum(COUNTS)), device=DEV)
    alone = [(x0[b:b + 1, :n].contiguous(), z[b:b + 1, :n].contiguous(), t[b:b + 1], noise[b:b + 1, :n].contiguous(),
              g_loss[b:b + 1, :n].contiguous()) for b, n in enumerate(COUNTS)]

    def ragged():
        tr.forward(sd, x0, z, t, noise, "l1", n_frames=COUNTS)
        return tr.backward(sd, g_loss)

    def uniform():
        tr.forward(sd, x0, z, t, noise, "l1")
        return tr.backward(sd, g_loss)

    def loop():
        out = None
        for xs, zs, ts, ns, gs in alone:
            tr.forward(sd, xs, zs, ts, ns, "l1")
            out = tr.backward(sd, gs)
        return out

    sides = {"uniform": uniform} if uniform_only else {"ragged": ragged, "uniform": uniform, "loop": loop}
    for _ in range(WARMUP):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, fn in sides.items():
            times[k].append(timed(fn, REPS))
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
    lib = os.environ.get("PD_ENGINE_LIB") or "the in-tree build"
    lines = [f"forward + backward of the diffusion loss (pred_noise, l1), default Denoiser, ({B}, {N}), counts {COUNTS}: ms per step, median of "
             f"{ROUNDS} alternating rounds of {REPS} steps (spread = (max - min) / median); library: {lib}"]
    names = {"ragged": "ragged  (8, 64) with counts  ", "uniform": "uniform (8, 64) without counts", "loop": "loop    8 calls at (1, n)    "}
    for k in sides:
        lines.append(f"  {names[k]}: {med[k]:7.3f} ms (spread {spread[k]:.1%})")
    print("\n".join(lines), flush=True)
    if argv:
        with open(argv[0], "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
