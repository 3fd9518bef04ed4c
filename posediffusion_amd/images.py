"""Training images on the engine (include/pd_engine_images.h): what the reference's ``datasets/co3d_v2.py:get_data`` does to
every frame on CPU workers -- a jittered square crop that may stick out of the picture, ``ToTensor`` + ``Resize(img_size, antialias=True)``,
and one ``ColorJitter`` / ``RandomGrayscale`` / ``RandomErasing`` draw per sequence -- for ALL frames of a batch in one call of
pd_train_images, from decoded ``uint8`` frames to the ``[F, 3, S, S]`` float tensor the backbone reads.

``prepare_training_images`` is the device half; ``draw_bbox_jitter`` and ``draw_colour`` are the random draws, made on the host (a
DataLoader worker can make them: they touch no GPU).  There is no CPU path and no fallback.

Draw order of ``draw_colour`` (torch's global generator, or ``generator``): one ``rand`` u, jitter applies when u <= p_jitter; if it
applies ``randperm(4)`` for the order, then one uniform each for brightness, contrast, saturation, hue, in that order; one ``rand`` for
grayscale (applies when < p_gray); with ``erase`` one ``rand`` (applies when < p) and then up to ten attempts of (uniform area fraction,
uniform log-ratio, and -- for an attempt that fits -- ``randint`` top, ``randint`` left).  The definitions follow torchvision's; identity
with torchvision's random stream is not claimed."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

STATUS_REASONS = {
    _lib.PD_IMG_BAD_SIDE: f"crop side outside 1 .. {_lib.PD_IMG_MAX_SIDE}",
    _lib.PD_IMG_BAD_SIZE: "height or width below 1, or a negative offset",
    _lib.PD_IMG_BAD_COLOUR: "colour index outside [-1, number of colour entries)",
    _lib.PD_IMG_BAD_ORDER: "the jitter order is no permutation of 0..3",
    _lib.PD_IMG_BAD_ERASE: "the erase rectangle does not lie inside the output",
}

NO_COLOUR = dict(jitter=0, order=(0, 1, 2, 3), brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, grayscale=0, erase=(0, 0, 0, 0))

_CACHE = {}   # device index -> dict(pinned, event, workspace): grown, never shrunk; one stream at a time per device


def square_box(box, padding=0.0, dtype=np.float32) -> np.ndarray:
    """The square xyxy box with the centre of ``box`` and half side = its larger half extent times (1 + padding), as ``dtype``."""
    box = np.array(box)
    lo, hi = box[:2], box[2:]
    mid, half = (lo + hi) / 2, max((hi - lo) / 2) * (1 + padding)
    return np.array([mid[0] - half, mid[1] - half, mid[0] + half, mid[1] + half], dtype=dtype)


def draw_bbox_jitter(bbox, jitter_scale=(0.8, 1.2), jitter_trans=(-0.07, 0.07)) -> np.ndarray:
    """The jittered crop box of ``Co3dDataset._jitter_bbox``: the float32 square around ``bbox``, its side scaled by one uniform draw from
    ``jitter_scale`` and its centre moved by a uniform draw of two from ``jitter_trans`` times the side (numpy's global generator, in that
    order); the upper-left corner is rounded, the lower-right one is the corner plus the rounded side.  Returns int xyxy, exactly square;
    it may leave the picture."""
    sq = square_box(np.asarray(bbox).astype(np.float32), dtype=np.float32)
    zoom = np.random.uniform(jitter_scale[0], jitter_scale[1])
    shift = np.random.uniform(jitter_trans[0], jitter_trans[1], size=2)
    side = sq[2] - sq[0]
    half = side / 2 * zoom
    corner = ((sq[:2] + sq[2:]) / 2 + shift * side - half).round().astype(int)
    return np.concatenate((corner, corner + np.round(2 * half).astype(int)))


def draw_colour(brightness=0.4, contrast=0.4, saturation=0.2, hue=0.1, p_jitter=0.65, p_gray=0.15, erase: Optional[dict] = None,
                generator: Optional[torch.Generator] = None) -> dict:
    """One sequence's colour draw (the module docstring states the order of the draws).  ``brightness`` / ``contrast`` / ``saturation`` b
    give factors uniform in [max(0, 1 - b), 1 + b], ``hue`` h a shift uniform in [-h, h] (ColorJitter's ranges).  ``erase``: None, or
    ``dict(image_size=S, p=0.1, scale=(0.02, 0.33), ratio=(0.3, 3.3))`` for RandomErasing's rectangle in an S x S output."""
    g = generator

    def u(lo, hi):
        return float(torch.empty(1).uniform_(lo, hi, generator=g))

    out = dict(NO_COLOUR)
    if float(torch.rand(1, generator=g)) <= p_jitter:
        out["jitter"] = 1
        out["order"] = tuple(int(v) for v in torch.randperm(4, generator=g))
        out["brightness"] = u(max(0.0, 1 - brightness), 1 + brightness)
        out["contrast"] = u(max(0.0, 1 - contrast), 1 + contrast)
        out["saturation"] = u(max(0.0, 1 - saturation), 1 + saturation)
        out["hue"] = u(-hue, hue)
    out["grayscale"] = int(float(torch.rand(1, generator=g)) < p_gray)
    if erase is not None:
        S = int(erase["image_size"])
        scale, ratio = erase.get("scale", (0.02, 0.33)), erase.get("ratio", (0.3, 3.3))
        if float(torch.rand(1, generator=g)) < erase.get("p", 0.1):
            for _ in range(10):
                area = S * S * u(scale[0], scale[1])
                aspect = math.exp(u(math.log(ratio[0]), math.log(ratio[1])))
                h, w = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
                if not (0 < h < S and 0 < w < S):
                    continue
                top = int(torch.randint(0, S - h + 1, (1,), generator=g))
                left = int(torch.randint(0, S - w + 1, (1,), generator=g))
                out["erase"] = (top, left, h, w)
                break
    return out


def colour_entry(d: Optional[dict]) -> _lib.pd_img_colour:
    d = dict(NO_COLOUR, **(d or {}))
    e = d.get("erase") or (0, 0, 0, 0)
    return _lib.pd_img_colour(int(d["jitter"]), (C.c_int32 * 4)(*[int(v) for v in d["order"]]), float(d["brightness"]), float(d["contrast"]),
                              float(d["saturation"]), float(d["hue"]), int(d["grayscale"]), int(e[0]), int(e[1]), int(e[2]), int(e[3]))


def _as_hwc_u8(fr, k: int) -> np.ndarray:
    if isinstance(fr, torch.Tensor):
        if fr.device.type != "cpu":
            raise ValueError(f"prepare_training_images: frame {k} is on {fr.device}; decoded frames are host arrays (they are packed and uploaded once)")
        fr = fr.numpy()
    fr = np.asarray(fr)
    if fr.dtype != np.uint8 or fr.ndim != 3 or fr.shape[2] != 3:
        raise ValueError(f"prepare_training_images: frame {k} must be uint8 [H, W, 3] (got {fr.dtype} {tuple(fr.shape)})")
    return np.ascontiguousarray(fr)


def _device_cache(dev: torch.device) -> dict:
    return _CACHE.setdefault(dev.index if dev.index is not None else torch.cuda.current_device(), dict(pinned=None, event=None, workspace=None))


def prepare_training_images(frames: Sequence, boxes, image_size: int = 224, sequence_of_frame=None, colour=None, fill: int = 0, device=None,
                            out: Optional[torch.Tensor] = None, strict: bool = True):
    """Crop, resize and colour F decoded frames in one launch on the current stream of ``device``.

    ``frames``: F ``uint8`` [H, W, 3] numpy arrays or CPU tensors of any sizes.  ``boxes`` [F, 4]: integer xyxy crop boxes, square, as
    ``draw_bbox_jitter`` returns them; they may lie partly or wholly outside their picture, where pixels read as ``fill`` (0 for the
    reference's plain crop, 255 for its white-background path).  ``colour``: None, one draw (a dict as ``draw_colour`` returns), or a
    list of draws, one per sequence; ``sequence_of_frame`` [F] then names each frame's entry (-1: none; default: entry 0 for every
    frame of a single draw).  ``out``: a contiguous float32 [F, 3, S, S] tensor on the device to write into.
    Limits: crop side <= 6144 (a status), ``image_size`` <= 1024 and F <= 65535 (``ValueError``).
    Frames and both tables travel in ONE pinned buffer and one upload; the pinned buffer and the kernel's workspace are kept per device
    (grown, never shrunk; use from one stream at a time).  Returns ``(images [F, 3, S, S], status [F] int32)``; a non-zero status
    (``STATUS_REASONS``) raises ``ValueError`` unless ``strict=False``, which also spares the device-to-host copy of ``status``."""
    if not torch.cuda.is_available():
        raise RuntimeError("prepare_training_images: the engine needs an AMD GPU (there is no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"prepare_training_images: device {dev} is not a GPU (there is no CPU fallback)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    S, F = int(image_size), len(frames)
    arrs = [_as_hwc_u8(fr, k) for k, fr in enumerate(frames)]
    bx = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    if bx.shape[0] != F:
        raise ValueError(f"prepare_training_images: {F} frames but {bx.shape[0]} boxes")
    if F and not np.array_equal(bx[:, 2] - bx[:, 0], bx[:, 3] - bx[:, 1]):
        raise ValueError("prepare_training_images: every crop box must be square (x1 - x0 == y1 - y0)")
    draws = [] if colour is None else ([colour] if isinstance(colour, dict) else list(colour))
    if sequence_of_frame is None:
        if len(draws) > 1:
            raise ValueError("prepare_training_images: several colour draws need sequence_of_frame")
        seq = [0 if draws else -1] * F
    else:
        seq = [int(v) for v in sequence_of_frame]
        if len(seq) != F:
            raise ValueError(f"prepare_training_images: sequence_of_frame holds {len(seq)} entries for {F} frames")
    if out is not None and (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.float32 or not out.is_contiguous()
                            or tuple(out.shape) != (F, 3, S, S)):
        raise ValueError(f"out must be a contiguous float32 tensor of shape {(F, 3, S, S)} on {dev}")
    images = out if out is not None else torch.empty(F, 3, S, S, device=dev)
    status = torch.empty(F, dtype=torch.int32, device=dev)
    lib = _lib.load()
    if F == 0:
        return images, status

    # one host buffer: frame table | colour table | pixels
    ftab = (_lib.pd_img_frame * F)()
    ctab = (_lib.pd_img_colour * max(1, len(draws)))(*[colour_entry(d) for d in draws])
    f_bytes, c_bytes = C.sizeof(ftab), (C.sizeof(_lib.pd_img_colour) * len(draws) + 7) // 8 * 8
    off = 0
    for k, a in enumerate(arrs):
        ftab[k] = _lib.pd_img_frame(off, a.shape[0], a.shape[1], int(bx[k, 0]), int(bx[k, 1]), int(bx[k, 2] - bx[k, 0]), seq[k])
        off += a.size
    total = f_bytes + c_bytes + off
    cache = _device_cache(dev)
    with torch.cuda.device(dev):
        if cache["event"] is not None:
            cache["event"].synchronize()          # the previous upload has left the pinned buffer
        if cache["pinned"] is None or cache["pinned"].numel() < total:
            cache["pinned"] = torch.empty(max(total, 1), dtype=torch.uint8).pin_memory()
        host = cache["pinned"].numpy()
        host[:f_bytes] = np.frombuffer(ftab, dtype=np.uint8)
        if draws:
            host[f_bytes:f_bytes + C.sizeof(_lib.pd_img_colour) * len(draws)] = np.frombuffer(ctab, dtype=np.uint8)[:C.sizeof(_lib.pd_img_colour) * len(draws)]
        p = f_bytes + c_bytes
        for a in arrs:
            host[p:p + a.size] = a.reshape(-1)
            p += a.size
        blob = torch.empty(total, dtype=torch.uint8, device=dev)
        blob.copy_(cache["pinned"][:total], non_blocking=True)
        cache["event"] = torch.cuda.Event()
        cache["event"].record()
        need = int(lib.pd_train_images_workspace_bytes(F, S))
        if need == 0:
            raise ValueError(f"prepare_training_images: image_size = {S} must lie in 1 .. {_lib.PD_IMG_MAX_SIZE} and the {F} frames must "
                             f"not exceed the {_lib.PD_IMG_MAX_FRAMES} of one call")
        if cache["workspace"] is None or cache["workspace"].numel() * 8 < need:
            cache["workspace"] = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
        ws = cache["workspace"]
        base = blob.data_ptr()
        _lib.check(lib.pd_train_images(base + f_bytes + c_bytes, base, F, (base + f_bytes) if draws else None, len(draws), S, int(fill),
                                       images.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                       torch.cuda.current_stream(dev).cuda_stream), "pd_train_images")
    if strict:
        bad = [(k, s) for k, s in enumerate(status.cpu().tolist()) if s != 0]
        if bad:
            raise ValueError("prepare_training_images: " + "; ".join(f"frame {k}: {STATUS_REASONS.get(s, f'status {s}')} (status {s})"
                                                                    for k, s in bad[:8]))
    return images, status
