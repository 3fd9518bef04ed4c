"""One training step's forward + backward on the trainer (pd_train_forward / pd_train_backward, include/pd_engine_train.h) against
PyTorch autograd on the same GPU running the reference's expression (oracle.pd_oracle.denoiser_forward in float32: rocBLAS GEMMs and
ATen elementwise kernels -- the only baseline that exists for this), at 64, 256 and 900 sequences of 20 frames.

One process: both sides hold the same weights and inputs; after warm-up they run in alternation, ROUNDS rounds of REPS steps each, timed
with events on the stream; the figure of a side is the median of its rounds, the spread its (max - min) / median.  The per-kernel share
of the engine's step comes from torch.profiler over one more step.  Recorded, not gated.
usage: python tests/perf/train_step_bench.py [out.txt]     (default out: profiles/train_step_timing.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pd_oracle as O                              # noqa: E402
from posediffusion_amd import synth                            # noqa: E402
from posediffusion_amd.host import get_trainer                 # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(64, 20), (256, 20), (900, 20)]
ROUNDS, REPS, WARMUP = 5, 3, 2


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main(out_path):
    diff = synth.make_diffuser(seed=0)
    synth.randomize_norm_and_bias_(diff.model)
    diff = diff.to(DEV).eval()
    params = dict(diff.model.named_parameters())
    tables = {n: b for n, b in diff.named_buffers(recurse=False)}
    lines = ["forward + backward of the diffusion loss (pred_noise, l1, loss.mean()), default Denoiser, ms per step: median of "
             f"{ROUNDS} alternating rounds of {REPS} steps (spread = (max - min) / median)",
             "engine = pd_train_forward + pd_train_backward (all parameter gradients and dz); torch = autograd of the reference's expression in float32 (rocBLAS)", ""]
    for B, N in SHAPES:
        g = torch.Generator().manual_seed(B)
        x0, noise = torch.randn(B, N, 9, generator=g).to(DEV), torch.randn(B, N, 9, generator=g).to(DEV)
        z, t = torch.randn(B, N, 384, generator=g).to(DEV), torch.randint(0, 100, (B,), generator=g).to(DEV)
        tr = get_trainer(diff.model, diff, B, N)
        sd = {k: p.detach() for k, p in params.items()}
        g_loss = torch.full((B, N, 9), 1.0 / (B * N * 9), device=DEV)

        def engine_step():
            tr.forward(sd, x0, z, t, noise, "l1")
            return tr.backward(sd, g_loss)

        zg = z.clone().requires_grad_()

        def torch_step():
            x_t = tables["sqrt_alphas_cumprod"][t].reshape(-1, 1, 1) * x0 + tables["sqrt_one_minus_alphas_cumprod"][t].reshape(-1, 1, 1) * noise
            with torch.device(DEV):                                # the oracle's constants (frequencies) are created on the GPU
                loss = (O.denoiser_forward(params, x_t, t, zg) - noise).abs().mean()
            return torch.autograd.grad(loss, list(params.values()) + [zg])

        for _ in range(WARMUP):
            engine_step()
            torch_step()
        torch.cuda.synchronize()
        te, tt = [], []
        for _ in range(ROUNDS):
            te.append(timed(engine_step, REPS))
            tt.append(timed(torch_step, REPS))
        me, mt = statistics.median(te), statistics.median(tt)
        lines.append(f"B={B:4d} N={N}: engine {me:8.2f} ms (spread {(max(te) - min(te)) / me:.1%})   torch {mt:8.2f} ms (spread {(max(tt) - min(tt)) / mt:.1%})"
                     f"   engine / torch = {me / mt:.2f}")
        try:
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                engine_step()
                torch.cuda.synchronize()
            dev_time = lambda e: getattr(e, "self_device_time_total", None) or getattr(e, "self_cuda_time_total", 0)   # noqa: E731
            rows = [(e.key, dev_time(e)) for e in prof.key_averages() if dev_time(e) > 0]
            total = sum(v for _, v in rows) or 1.0
            for k, v in sorted(rows, key=lambda r: -r[1])[:8]:
                lines.append(f"      {100.0 * v / total:5.1f} %  {k[:110]}")
        except Exception as exc:                                   # the figures above stand without the breakdown
            lines.append(f"      (per-kernel share unavailable: {type(exc).__name__}: {exc})")
        print("\n".join(lines[-10:]), flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "train_step_timing.txt"))
