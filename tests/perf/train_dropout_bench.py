"""What dropout costs a training step on the trainer: forward + backward with p = 0.1 at all four sites of every encoder layer
(pd_train_forward_dropout / pd_train_backward, include/pd_engine_train.h) against the SAME trainer's step without dropout, and against
PyTorch autograd of the reference's expression with its nn.TransformerEncoder in .train() mode (torch's own dropout kernels), at 64, 256
and 900 sequences of 20 frames.  Each single site is timed too, so that a cost can be given to the site that causes it.

Method of tests/perf/train_step_bench.py: one process, the same weights and inputs on every side, alternating rounds after warm-up, ROUNDS
rounds of REPS steps timed with events on the stream; a side's figure is the median of its rounds, its spread (max - min) / median.
Recorded, not gated.
usage: python tests/perf/train_dropout_bench.py [out.txt]     (default out: profiles/train_dropout_timing.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pd_oracle as O                              # noqa: E402
from posediffusion_amd import synth                            # noqa: E402
from posediffusion_amd.host import get_trainer                 # noqa: E402
from posediffusion_amd.train import ALL, DROPOUT_SITES         # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(64, 20), (256, 20), (900, 20)]
ROUNDS, REPS, WARMUP = 5, 3, 2
P = 0.1


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
    diff = diff.to(DEV)
    den = diff.model
    params = dict(den.named_parameters())
    tables = {n: b for n, b in diff.named_buffers(recurse=False)}
    lines = [f"forward + backward of the diffusion loss (pred_noise, l1, loss.mean()), default Denoiser, dropout p = {P}, ms per step: median of "
             f"{ROUNDS} alternating rounds of {REPS} steps (spread = (max - min) / median)",
             "plain = pd_train_forward + pd_train_backward (the step without dropout); all / attn / resid1 / ff / resid2 = pd_train_forward_dropout at "
             "those sites + pd_train_backward;", "torch = autograd of the reference's expression in float32 with nn.TransformerEncoder in .train() mode", ""]
    for B, N in SHAPES:
        g = torch.Generator().manual_seed(B)
        x0, noise = torch.randn(B, N, 9, generator=g).to(DEV), torch.randn(B, N, 9, generator=g).to(DEV)
        z, t = torch.randn(B, N, 384, generator=g).to(DEV), torch.randint(0, 100, (B,), generator=g).to(DEV)
        tr = get_trainer(den, diff, B, N)
        sd = {k: p.detach() for k, p in params.items()}
        g_loss = torch.full((B, N, 9), 1.0 / (B * N * 9), device=DEV)
        counter = [0]

        def engine_step(sites):
            def step():
                counter[0] += 1
                tr.forward(sd, x0, z, t, noise, "l1", dropout_p=P if sites else 0.0, dropout_sites=sites or ALL, seed=B, step=counter[0])
                return tr.backward(sd, g_loss)
            return step

        zg = z.clone().requires_grad_()
        den.train()

        def torch_step():
            x_t = tables["sqrt_alphas_cumprod"][t].reshape(-1, 1, 1) * x0 + tables["sqrt_one_minus_alphas_cumprod"][t].reshape(-1, 1, 1) * noise
            with torch.device(DEV):                                # the oracle's constants (frequencies) are created on the GPU
                t_emb = O.timestep_embedding(t, params)[:, None, :].expand(-1, N, -1)
                pivot = torch.zeros_like(zg[..., :1])
                pivot[:, 0] = 1.0
                h = torch.cat([O.harmonic_embedding(x_t), t_emb, zg, pivot], dim=-1) @ params["_first.weight"].T + params["_first.bias"]
                h = den._trunk(h)                                  # torch's encoder layers with their dropout
                a = torch.relu(O._layer_norm(h @ params["_last.0.weight"].T + params["_last.0.bias"], params["_last.1.weight"], params["_last.1.bias"]))
                out = a @ params["_last.3.weight"].T + params["_last.3.bias"]
                loss = (out - noise).abs().mean()
            return torch.autograd.grad(loss, list(params.values()) + [zg])

        sides = {"plain": engine_step(0), "all": engine_step(ALL), **{k: engine_step(v) for k, v in DROPOUT_SITES.items()}, "torch": torch_step}
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
        lines.append(f"B={B:4d} N={N}: plain {med['plain']:8.2f} ms (spread {spread['plain']:.1%})   all sites {med['all']:8.2f} ms (spread {spread['all']:.1%})"
                     f"   all / plain = {med['all'] / med['plain']:.3f}   torch .train() {med['torch']:8.2f} ms (spread {spread['torch']:.1%})"
                     f"   all / torch = {med['all'] / med['torch']:.2f}")
        lines.append("      one site alone / plain: " + "   ".join(f"{k} {med[k] / med['plain']:.3f}" for k in DROPOUT_SITES))
        try:
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                sides["all"]()
                torch.cuda.synchronize()
            dev_time = lambda e: getattr(e, "self_device_time_total", None) or getattr(e, "self_cuda_time_total", 0)   # noqa: E731
            rows = [(e.key, dev_time(e)) for e in prof.key_averages() if dev_time(e) > 0]
            total = sum(v for _, v in rows) or 1.0
            for k, v in sorted(rows, key=lambda r: -r[1])[:8]:
                lines.append(f"      {100.0 * v / total:5.1f} %  {k[:110]}")
        except Exception as exc:                                   # the figures above stand without the breakdown
            lines.append(f"      (per-kernel share unavailable: {type(exc).__name__}: {exc})")
        print("\n".join(lines[-11:]), flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "train_dropout_timing.txt"))
