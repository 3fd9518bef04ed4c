"""Not a test, no threshold: the training-image path at the reference's workload -- 512 frames of 1000 x 1800 -> 224 with the colour draw on
(cfgs/default_train.yaml: max_images 512, img_size 224, color_aug True) -- as ONE pd_train_images call against torch on the same GPU
doing, per frame, crop + ``F.interpolate(antialias=True)`` + the same colour operations (tests/train_images_checks.py in fp32 on the
device).  Both start from the frames already on the device, one process, interleaved rounds, device events around each side (the
engine's window is 40 calls back to back, reported per call).  Decoding, the host-side packing and the upload are outside both figures.

    python tests/perf/train_images_bench.py [out.txt] [n_frames]        (writes profiles/train_images.txt by default)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import train_images_checks as IC  # noqa: E402
from posediffusion_amd import _lib  # noqa: E402
from posediffusion_amd.images import colour_entry, draw_bbox_jitter, draw_colour  # noqa: E402

H, W, S, FRAMES_PER_SEQ, ROUNDS, WARM, ENGINE_REPS = 1000, 1800, 224, 16, 7, 2, 40


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "train_images.txt")
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    if not torch.cuda.is_available():
        raise SystemExit("train_images_bench needs an AMD GPU")
    dev = torch.device("cuda:0")
    np.random.seed(0)
    g = torch.Generator().manual_seed(0)
    n_seq = (n + FRAMES_PER_SEQ - 1) // FRAMES_PER_SEQ
    draws = [draw_colour(generator=g) for _ in range(n_seq)]
    for d in draws[::2]:                       # every other sequence jitters for certain: the timed work does not hang on the seed
        d.update(draw_colour(p_jitter=1.0, generator=g))
    left = (W - H) // 2
    boxes = np.stack([draw_bbox_jitter(np.array([left, 0, left + H, H])) for _ in range(n)])
    # eight distinct pictures repeated: 2.8 GB of pixels on the device, well past the 256 MB Infinity Cache
    pics = [torch.from_numpy(IC.picture(H, W, seed=k)) for k in range(8)]
    pixels = torch.cat([pics[k % 8].reshape(-1) for k in range(n)]).to(dev)
    ftab = (_lib.pd_img_frame * n)()
    for k in range(n):
        ftab[k] = _lib.pd_img_frame(k * H * W * 3, H, W, int(boxes[k, 0]), int(boxes[k, 1]), int(boxes[k, 2] - boxes[k, 0]), k // FRAMES_PER_SEQ)
    ftab_d = torch.from_numpy(np.frombuffer(ftab, dtype=np.uint8).copy()).to(dev)
    ctab = (_lib.pd_img_colour * n_seq)(*[colour_entry(d) for d in draws])
    ctab_d = torch.from_numpy(np.frombuffer(ctab, dtype=np.uint8).copy()).to(dev)
    out = torch.empty(n, 3, S, S, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws = torch.empty(lib.pd_train_images_workspace_bytes(n, S) // 8, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def engine():
        _lib.check(lib.pd_train_images(pixels.data_ptr(), ftab_d.data_ptr(), n, ctab_d.data_ptr(), n_seq, S, 0, out.data_ptr(), status.data_ptr(),
                                       ws.data_ptr(), ws.numel() * 8, stream), "pd_train_images")

    frames_d = pixels.view(n, H, W, 3)
    ref = torch.empty_like(out)

    def torch_side():
        for k in range(n):
            x0, y0, x1, y1 = (int(v) for v in boxes[k])
            crop = frames_d[k, max(y0, 0):min(y1, H), max(x0, 0):min(x1, W)].permute(2, 0, 1).float().div(255)
            crop = F.pad(crop, (max(-x0, 0), max(x1 - W, 0), max(-y0, 0), max(y1 - H, 0)))
            x = F.interpolate(crop[None], size=(S, S), mode="bilinear", antialias=True)[0]
            ref[k] = IC.apply_colour(x, draws[k // FRAMES_PER_SEQ])

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(WARM):
        engine()
        torch_side()
    torch.cuda.synchronize()
    assert int(status.abs().max()) == 0
    t_eng, t_ref = [], []
    for _ in range(ROUNDS):
        t_eng.append(timed(lambda: [engine() for _ in range(ENGINE_REPS)]) / ENGINE_REPS)
        t_ref.append(timed(torch_side))
    diff = (out - ref).abs().max().item()
    sides = boxes[:, 2] - boxes[:, 0]
    yy = np.clip(boxes[:, 3], 0, H) - np.clip(boxes[:, 1], 0, H)
    xx = np.clip(boxes[:, 2], 0, W) - np.clip(boxes[:, 0], 0, W)
    read = float((yy * xx * 3).sum())                      # bytes of the crops inside their pictures, each once
    med = lambda v: float(np.median(v))  # noqa: E731
    lines = [
        f"training images: {n} frames of {H} x {W} -> {S}, crop sides {sides.min()} .. {sides.max()} (jitter 0.8 .. 1.2 of the centre box), "
        f"{n_seq} colour draws ({sum(d['jitter'] for d in draws)} jitter, {sum(d['grayscale'] for d in draws)} grayscale)",
        f"one process on {torch.cuda.get_device_name(0)}, {WARM} warm-up rounds, {ROUNDS} interleaved timed rounds, device events; a timed window is {ENGINE_REPS} engine calls "
        f"back to back (reported per call) or one torch pass; frames on the device before the clock starts: decoding, packing into the pinned buffer "
        f"and the upload are not in either figure",
        f"pd_train_images (2 kernels)        median {med(t_eng):8.3f} ms   min {min(t_eng):8.3f}   max {max(t_eng):8.3f}",
        f"torch per frame (crop, pad, F.interpolate(antialias=True), colour ops; issued from Python)  median {med(t_ref):8.3f} ms   min {min(t_ref):8.3f}   max {max(t_ref):8.3f}",
        f"ratio torch / engine               {med(t_ref) / med(t_eng):8.1f} x",
        f"crop bytes read once {read / 1e9:.3f} GB + {out.numel() * 4 / 1e9:.3f} GB written (and re-read / re-written by the colour kernel for its frames): "
        f"{read / 1e9 / (med(t_eng) * 1e-3):.0f} GB/s of crop bytes over the whole call",
        f"largest |engine - torch fp32| over the batch {diff:.3e} (torch's fp32 resize forms its centres in fp32: DESIGN 3.14)",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
