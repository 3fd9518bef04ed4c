"""Per-sequence timesteps in one pass against the single-t step and against the grouped loop they replace, at (B, N) = (64, 20) with 64
random timesteps (1 280 token rows: the large-batch path in the engine's default mode).

  (a) pd_denoise_step at a single t            (b) pd_denoise_step_t            (c) pd_p_losses (q_sample + denoiser + loss)
  (d) the grouped loop Denoiser.forward ran before pd_denoise_step_t existed: one pd_denoise_step per distinct t, rows gathered and
      scattered through torch (kept here as a local helper)

One process, one box: the four are timed in alternation, ROUNDS rounds of REPS calls each between device events, every shape warmed up
first; the figure of a variant is the median of its rounds, the spread its (max - min) / median.
usage: python tests/perf/p_losses_bench.py [out.txt]  -> the table (also written to out.txt, default profiles/p_losses_timing.txt) + one JSON line"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from posediffusion_amd import _lib, synth                     # noqa: E402
from posediffusion_amd.host import get_engine                 # noqa: E402

DEV = torch.device("cuda:0")
B, N, T = 64, 20, 100
ROUNDS, REPS = 15, 20


def grouped_loop(eng, x, z, t):
    """Denoiser.forward(x, t[B], z) as the parent commit ran it: one launch group per distinct t."""
    out = torch.empty_like(x)
    for s in t.unique().tolist():
        sel = (t == s).nonzero().flatten()
        out[sel] = eng.denoise(x[sel], z[sel], int(s))
    return out


def main():
    if not torch.cuda.is_available():
        raise RuntimeError("p_losses_bench.py measures on an AMD GPU; none is visible")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "p_losses_timing.txt")
    diff = synth.make_diffuser(seed=0)
    synth.randomize_norm_and_bias_(diff.model)
    diff = diff.to(DEV)
    eng = get_engine(diff.model, diff, B, N)
    lib, h, stream = eng.lib, eng._h, torch.cuda.current_stream(DEV).cuda_stream
    g = torch.Generator().manual_seed(0)
    x, noise = torch.randn(B, N, 9, generator=g).to(DEV), torch.randn(B, N, 9, generator=g).to(DEV)
    z = synth.make_z(B, N).to(DEV)
    t = torch.randint(0, T, (B,), generator=g).to(DEV)
    o = [torch.empty_like(x) for _ in range(4)]
    p = lambda v: v.data_ptr()                                 # noqa: E731
    variants = {
        "a pd_denoise_step (single t)": lambda: _lib.check(lib.pd_denoise_step(h, p(x), p(z), 50, B, N, p(o[0]), stream)),
        "b pd_denoise_step_t": lambda: _lib.check(lib.pd_denoise_step_t(h, p(x), p(z), p(t), B, N, p(o[0]), stream)),
        "c pd_p_losses": lambda: _lib.check(lib.pd_p_losses(h, p(x), p(z), p(t), p(noise), B, N, 1, p(o[0]), p(o[1]), p(o[2]), p(o[3]), stream)),
        "d grouped loop (one step per distinct t)": lambda: grouped_loop(eng, x, z, t),
    }
    assert torch.equal(grouped_loop(eng, x, z, t) * 0, eng.denoise_t(x, z, t) * 0)      # both run; finite
    for fn in variants.values():                               # warm-up: code objects, allocator, every shape of the grouped loop
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            reps = REPS if not k.startswith("d") else max(REPS // 10, 2)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / reps * 1e3)  # us per call
    eng.check_async()
    med = {k: statistics.median(v) for k, v in times.items()}
    a, b, c, d = (med[k] for k in variants)
    lines = [f"(B, N) = ({B}, {N}), {len(t.unique())} distinct timesteps of {B}; split mode {eng.get_option(_lib.PD_OPT_DENOISER_SPLIT)}; "
             f"{ROUNDS} interleaved rounds, median us per call (spread = (max - min) / median)"]
    for k, v in times.items():
        lines.append(f"  {k:44s} {med[k]:10.1f} us   spread {(max(v) - min(v)) / med[k]:.2f}")
    lines.append(f"  b / a = {b / a:.3f}    c / a = {c / a:.3f}    d / b = {d / b:.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    print(json.dumps({"us": {k[0]: round(v, 1) for k, v in med.items()}, "b_over_a": round(b / a, 3), "c_over_a": round(c / a, 3),
                      "d_over_b": round(d / b, 2)}))


if __name__ == "__main__":
    main()
