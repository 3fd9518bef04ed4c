"""One training step's forward + backward on the trainer at 65 ... 256 frames per sequence (PD_TR_OPT_MAX_FRAMES: the key-tiled attention
kernels pd_tr_lattn_kernel, pd_tr_lattn_bwd_rows_kernel, pd_tr_lattn_bwd_keys_kernel) against PyTorch autograd on the same GPU running the
reference's expression in float32, with and without dropout 0.1 at all four sites, at 64 x 65, 40 x 128 and 20 x 256 sequences x frames
(4 160 to 5 120 token rows: next to the 256 x 20 row of profiles/train_step_timing.txt).

The method of tests/perf/train_step_bench.py: one process, both sides hold the same weights and inputs; after warm-up they run in
alternation, ROUNDS rounds of REPS steps each, timed with events on the stream; the figure of a side is the median of its rounds, the
spread its (max - min) / median.  The per-kernel share of the engine's step comes from torch.profiler over one more step; the shares of
the three attention kernels and of pd_tr_gemm_kernel are summed out.  Recorded, not gated.
usage: python tests/perf/train_long_bench.py [out.txt]     (default out: profiles/train_long_timing.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pd_oracle as O                              # noqa: E402
from posediffusion_amd import synth                            # noqa: E402
from posediffusion_amd.host import get_trainer                 # noqa: E402
from posediffusion_amd.train import ALL                        # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(64, 65), (40, 128), (20, 256)]
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


def kernel_shares(step):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    dev_time = lambda e: getattr(e, "self_device_time_total", None) or getattr(e, "self_cuda_time_total", 0)   # noqa: E731
    rows = [(e.key, dev_time(e)) for e in prof.key_averages() if dev_time(e) > 0]
    total = sum(v for _, v in rows) or 1.0
    return [(k, v / total) for k, v in sorted(rows, key=lambda r: -r[1])]


def main(out_path):
    diff = synth.make_diffuser(seed=0)
    synth.randomize_norm_and_bias_(diff.model)
    diff = diff.to(DEV)
    den = diff.model
    params = dict(den.named_parameters())
    tables = {n: b for n, b in diff.named_buffers(recurse=False)}
    lines = ["forward + backward of the diffusion loss (pred_noise, l1, loss.mean()), default Denoiser, 65 ... 256 frames per sequence, ms per step: "
             f"median of {ROUNDS} alternating rounds of {REPS} steps (spread = (max - min) / median)",
             "engine = pd_train_forward(_dropout) + pd_train_backward with PD_TR_OPT_MAX_FRAMES = 256 (key-tiled attention); torch = autograd of the "
             f"reference's expression in float32 (nn.TransformerEncoder in .eval() / .train() mode); dropout p = {P} at all four sites", ""]
    for B, N in SHAPES:
        g = torch.Generator().manual_seed(B)
        x0, noise = torch.randn(B, N, 9, generator=g).to(DEV), torch.randn(B, N, 9, generator=g).to(DEV)
        z, t = torch.randn(B, N, 384, generator=g).to(DEV), torch.randint(0, 100, (B,), generator=g).to(DEV)
        tr = get_trainer(den, diff, B, N, max_frames=256)
        sd = {k: p.detach() for k, p in params.items()}
        g_loss = torch.full((B, N, 9), 1.0 / (B * N * 9), device=DEV)
        counter = [0]

        def engine_step(p):
            def step():
                counter[0] += 1
                tr.forward(sd, x0, z, t, noise, "l1", dropout_p=p, dropout_sites=ALL, seed=B, step=counter[0])
                return tr.backward(sd, g_loss)
            return step

        zg = z.clone().requires_grad_()

        def torch_step(train):
            def step():
                den.train(train)
                x_t = tables["sqrt_alphas_cumprod"][t].reshape(-1, 1, 1) * x0 + tables["sqrt_one_minus_alphas_cumprod"][t].reshape(-1, 1, 1) * noise
                with torch.device(DEV):                            # the oracle's constants (frequencies) are created on the GPU
                    t_emb = O.timestep_embedding(t, params)[:, None, :].expand(-1, N, -1)
                    pivot = torch.zeros_like(zg[..., :1])
                    pivot[:, 0] = 1.0
                    h = torch.cat([O.harmonic_embedding(x_t), t_emb, zg, pivot], dim=-1) @ params["_first.weight"].T + params["_first.bias"]
                    h = den._trunk(h)
                    a = torch.relu(O._layer_norm(h @ params["_last.0.weight"].T + params["_last.0.bias"], params["_last.1.weight"], params["_last.1.bias"]))
                    loss = (a @ params["_last.3.weight"].T + params["_last.3.bias"] - noise).abs().mean()
                return torch.autograd.grad(loss, list(params.values()) + [zg])
            return step

        sides = {"engine": engine_step(0.0), "engine_drop": engine_step(P), "torch": torch_step(False), "torch_drop": torch_step(True)}
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
        lines.append(f"B={B:3d} N={N:3d} ({B * N} rows): engine {med['engine']:7.2f} ms (spread {spread['engine']:.1%})   torch {med['torch']:7.2f} ms "
                     f"(spread {spread['torch']:.1%})   engine / torch = {med['engine'] / med['torch']:.2f}")
        lines.append(f"      dropout {P}:        engine {med['engine_drop']:7.2f} ms (spread {spread['engine_drop']:.1%})   torch {med['torch_drop']:7.2f} ms "
                     f"(spread {spread['torch_drop']:.1%})   engine / torch = {med['engine_drop'] / med['torch_drop']:.2f}")
        for label, key in (("no dropout", "engine"), (f"dropout {P}", "engine_drop")):
            try:
                shares = kernel_shares(sides[key])
                attn = {n: sum(v for k, v in shares if n in k) for n in ("pd_tr_lattn_kernel", "pd_tr_lattn_bwd_rows_kernel", "pd_tr_lattn_bwd_keys_kernel")}
                gemm = sum(v for k, v in shares if "pd_tr_gemm_kernel" in k)
                lines.append(f"      {label}: attention {100 * sum(attn.values()):5.1f} % of the step (forward {100 * attn['pd_tr_lattn_kernel']:.1f} %, backward rows "
                             f"{100 * attn['pd_tr_lattn_bwd_rows_kernel']:.1f} %, backward keys {100 * attn['pd_tr_lattn_bwd_keys_kernel']:.1f} %); "
                             f"pd_tr_gemm_kernel {100 * gemm:5.1f} %")
                for k, v in shares[:6]:
                    lines.append(f"          {100.0 * v:5.1f} %  {k[:110]}")
            except Exception as exc:                               # the figures above stand without the breakdown
                lines.append(f"      (per-kernel share unavailable: {type(exc).__name__}: {exc})")
        print("\n".join(lines[-18:]), flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "train_long_timing.txt"))
