"""The optimiser step (include/pd_engine_optim.h) on the full training parameter set: the 108 tensors of the default 8-layer denoiser and the
150 of the DINO ViT-S/16, 258 live fp32 tensors, with random gradients; global-norm clipping at 1 and AdamW.

Three contestants in ONE process, in interleaved rounds on the same GPU, each on its own copy of the parameters and gradients:
  engine         EngineAdamW.step(max_grad_norm=1)                                   (norm pass + fused clip-and-update pass)
  torch foreach  torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(foreach=True)
  torch fused    torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(fused=True)
Each timing is REPS back-to-back steps between two device events after a warm-up of all three; the table gives every round, the median
and the spread, and the host time to ISSUE a step (no synchronisation inside the window: when it exceeds the device time, the step is
bound by the host) -- and the time of the same REPS steps queued behind a few large matrix products, where the host has issued them all
before the device starts on the first: the device time alone.  Roof: the update reads p, g, m, v and writes p, m, v (28 B per element), the norm pass reads g once more: 32 B per
element at the 6.3 TB/s of a streaming kernel.  Recorded, not gated.

usage: python tests/perf/optim_step_bench.py [out.txt]   (default profiles/optim_step.txt)"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import vit_oracle as VO                                             # noqa: E402
from posediffusion_amd import synth                                             # noqa: E402
from posediffusion_amd.optim import EngineAdamW                                 # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS, REPS, WARMUP = 5, 10, 3
STREAM_BYTES_PER_S, BYTES_PER_ELEMENT = 6.3e12, 32


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    host = (time.perf_counter() - t0) / reps * 1e3
    e1.synchronize()
    return e0.elapsed_time(e1) / reps, host      # ms per step on the device, ms per step to issue


def _timed_queued(fn, reps, busy):
    """ms per step on the device when the steps wait in the queue behind `busy` (the host is done issuing before they start)"""
    e0, e1, issued = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event()
    torch.cuda.synchronize()
    busy()
    issued.record()
    e0.record()
    for _ in range(reps):
        fn()
    ahead = not issued.query()                   # the matrix products were still running when the last step was issued
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps if ahead else float("nan")


def _parameter_set(seed):
    shapes = [tuple(p.shape) for p in synth.make_diffuser(seed=0).model.parameters()] + [tuple(p.shape) for p in VO.make_vit(seed=0).parameters()]
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter((0.05 * torch.randn(s, generator=g)).to(DEV)) for s in shapes]
    for p in params:
        p.grad = (1e-2 * torch.randn(p.shape, generator=g)).to(DEV)
    return params


def main(out_path):
    if not torch.cuda.is_available():
        raise RuntimeError("optim_step_bench needs an AMD GPU: a timing taken elsewhere says nothing about it")
    sets = {k: _parameter_set(7) for k in ("engine", "torch foreach", "torch fused")}
    n, numel = len(sets["engine"]), sum(p.numel() for p in sets["engine"])
    kw = dict(lr=1e-4, weight_decay=1e-2)
    eng = EngineAdamW(sets["engine"], max_grad_norm=1.0, **kw)
    foreach = torch.optim.AdamW(sets["torch foreach"], foreach=True, **kw)
    fused = torch.optim.AdamW(sets["torch fused"], fused=True, **kw)

    def torch_step(opt, params):
        def step():
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
        return step

    steps = {"engine": eng.step, "torch foreach": torch_step(foreach, sets["torch foreach"]), "torch fused": torch_step(fused, sets["torch fused"])}
    for _ in range(WARMUP):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    far = max(float((a - b).detach().abs().max()) for a, b in zip(sets["engine"], sets["torch fused"]))
    times = {k: [] for k in steps}
    hosts = {k: [] for k in steps}
    queued = {k: [] for k in steps}
    a = torch.randn(8192, 8192, device=DEV)

    def busy():
        for _ in range(40):                      # several times the slowest contestant's time to issue its steps
            a @ a

    for _ in range(ROUNDS):
        for k, fn in steps.items():
            dev_ms, host_ms = _timed(fn, REPS)
            times[k].append(dev_ms)
            hosts[k].append(host_ms)
            queued[k].append(_timed_queued(fn, REPS, busy))
    roof_ms = numel * BYTES_PER_ELEMENT / STREAM_BYTES_PER_S * 1e3
    lines = [f"optimiser step, clip at 1 + AdamW, {n} tensors of {numel} fp32 values ({numel * 4 / 2 ** 20:.0f} MiB each of p, g, m, v); "
             f"{torch.cuda.get_device_name(0)}",
             f"{ROUNDS} interleaved rounds of {REPS} steps after {WARMUP} warm-up steps of all; ms per step between device events, and to issue on the host",
             f"largest |p_engine - p_fused| after the warm-up steps: {far:.3e} (lr {kw['lr']:g})",
             f"roof: {BYTES_PER_ELEMENT} B per element at {STREAM_BYTES_PER_S / 1e12:.1f} TB/s = {roof_ms:.3f} ms"]
    for k, v in times.items():
        med = statistics.median(v)
        lines.append(f"{k:13s} median {med:7.3f} ms  (min {min(v):.3f}, max {max(v):.3f}; rounds {' '.join(f'{t:.3f}' for t in v)})  "
                     f"host issue median {statistics.median(hosts[k]):.3f} ms;  device alone median {statistics.median(queued[k]):.3f} ms "
                     f"(rounds {' '.join(f'{t:.3f}' for t in queued[k])})")
    if any(t != t for v in queued.values() for t in v):
        lines.append("(device alone nan: the host was not through issuing the steps when the device reached them)")
    e = statistics.median(times["engine"])
    lines.append(f"engine: {roof_ms / e:.2f} of the roof as timed, {roof_ms / statistics.median(queued['engine']):.2f} of it on the device alone; "
                 f"engine / torch foreach {e / statistics.median(times['torch foreach']):.2f}, "
                 f"engine / torch fused {e / statistics.median(times['torch fused']):.2f} (medians)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "optim_step.txt"))
