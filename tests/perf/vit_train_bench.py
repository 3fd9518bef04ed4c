"""The backbone trainer (include/pd_engine_vit_train.h) at the reference's training shape: forward + backward of the 12-block DINO ViT-S/16
for 20 images of 224 x 224 at the scales 1, 1/2, 1/3 (197 + 50 + 17 tokens per image, 5 280 token rows), every parameter gradient.

Two contestants in ONE process, in interleaved rounds on the same GPU and the same weights and images:
  engine   VitTrainer.forward + VitTrainer.backward (exact fp32, hand-written kernels, no weight copy)
  torch    fp32 autograd of oracle/vit_oracle.DinoViT under tests/vit_train_checks.multiscale (rocBLAS / MIOpen eager kernels)
Each timing is REPS back-to-back steps between two device events after a warm-up of both; the table gives every round, the median
and the spread.  Recorded, not gated: the engine's GEMM is the trainer's exact-fp32 64 x 64 tile, not a tuned one.  FLOP figure: the
matrix products of the forward (2 x rows x weights, attention 4 x tokens^2 x 384 per image and block) times three for forward + backward.

usage: python tests/perf/vit_train_bench.py [out.txt]   (default profiles/vit_train.txt)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_train_checks as VC                                                    # noqa: E402
from oracle import vit_oracle as VO                                             # noqa: E402
from posediffusion_amd.vit_train import VitTrainer, shape_from_module, token_rows   # noqa: E402

DEV = torch.device("cuda:0")
N_IMG, SIDE, SCALES = 20, 224, (1, 1 / 2, 1 / 3)
ROUNDS, REPS, WARMUP = 5, 10, 2         # a timed window is 10 steps: 0.4 - 0.6 s


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps      # ms per step


def _flops():
    total = 0.0
    for sf in SCALES:
        side = SIDE if sf == 1 else int(SIDE * sf)
        P = (side // 16) ** 2
        T, rows = P + 1, N_IMG * (P + 1)
        total += 2.0 * N_IMG * P * 768 * 384
        total += 12 * (2.0 * rows * 384 * (3 * 384 + 384 + 2 * 1536) + 4.0 * N_IMG * T * T * 384)
    return 3.0 * total


def main(out_path):
    if not torch.cuda.is_available():
        raise RuntimeError("vit_train_bench needs an AMD GPU: a timing taken elsewhere says nothing about it")
    net = VO.make_vit(seed=0).to(DEV)
    g = torch.Generator().manual_seed(5)
    images = torch.rand(N_IMG, 3, SIDE, SIDE, generator=g).to(DEV)
    g_z = torch.randn(N_IMG, 384, generator=g).to(DEV)
    params = {k: v.detach() for k, v in net.named_parameters()}
    tr = VitTrainer(shape_from_module(net), N_IMG, N_IMG * token_rows(SIDE, SIDE, SCALES), len(SCALES), device=DEV)
    mean = torch.tensor(VO.RESNET_MEAN, device=DEV).view(1, 3, 1, 1)
    std = torch.tensor(VO.RESNET_STD, device=DEV).view(1, 3, 1, 1)

    def engine_step():
        tr.forward(params, images, SCALES)
        return tr.backward(params, g_z)

    def torch_step():
        img = (images - mean) / std
        feats = None
        for sf in SCALES:
            inp = img if sf == 1 else torch.nn.functional.interpolate(img, scale_factor=sf, mode="bilinear", align_corners=False)
            f = net(inp)
            feats = f if feats is None else feats + f
        z = feats / len(SCALES)
        return torch.autograd.grad((z * g_z).sum(), list(net.parameters()))

    for _ in range(WARMUP):
        ge, gt = engine_step(), torch_step()
    torch.cuda.synchronize()
    names = [n for n, _ in net.named_parameters()]
    worst = max(VC.grad_dist(ge[n], t) for n, t in zip(names, gt))
    times = {"engine": [], "torch": []}
    for _ in range(ROUNDS):
        times["engine"].append(_timed(engine_step, REPS))
        times["torch"].append(_timed(torch_step, REPS))
    fl = _flops()
    lines = [f"backbone trainer, forward + backward, {N_IMG} images of {SIDE} x {SIDE} at scales 1, 1/2, 1/3 "
             f"({N_IMG * token_rows(SIDE, SIDE, SCALES)} token rows, 12 blocks); {torch.cuda.get_device_name(0)}",
             f"{ROUNDS} interleaved rounds of {REPS} steps after {WARMUP} warm-up steps of both; ms per step",
             f"largest distance between the two sets of gradients (max|a - b| / max|b| per tensor): {worst:.3e}"]
    for k, v in times.items():
        med = statistics.median(v)
        lines.append(f"{k:7s} median {med:8.2f} ms  (min {min(v):.2f}, max {max(v):.2f}; rounds {' '.join(f'{t:.2f}' for t in v)})  "
                     f"{fl / med / 1e9:7.1f} TFLOP/s of matrix products")
    lines.append(f"engine / torch (medians): {statistics.median(times['engine']) / statistics.median(times['torch']):.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    tr.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vit_train.txt"))
