"""Yardstick of the training-image kernels (include/pd_engine_images.h) and the case tables of their tests: the padded
crop, the closed-form weights of torch's antialiased bilinear resize, and torchvision's float-tensor colour operations, all in a dtype
of the caller's choice (fp64: the yardstick; fp32: the restatement whose own error sets the colour bound)."""
import gzip
import itertools
import json
import math
import os

import numpy as np
import torch
from PIL import Image

EPS24 = 2.0 ** -24


# ---- crop ---------------------------------------------------------------------------------------------------------------------------
def padded_crop(img, x0, y0, side, fill):
    """[side, side, 3] uint8: img[y0 : y0 + side, x0 : x0 + side] with everything outside the picture = fill."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    out = np.full((side, side, 3), fill, dtype=np.uint8)
    ya, yb, xa, xb = max(0, y0), min(H, y0 + side), max(0, x0), min(W, x0 + side)
    if yb > ya and xb > xa:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = img[ya:yb, xa:xb]
    return out


# ---- resize -------------------------------------------------------------------------------------------------------------------------
def aa_weights(side, S):
    """Dense [S, side] fp64 weights of _upsample_bilinear2d_aa (align_corners=False), the closed form, and the largest tap count."""
    scale = side / S
    support = max(scale, 1.0)
    inv = 1.0 / support
    Wm = torch.zeros(S, side, dtype=torch.float64)
    taps = 0
    for i in range(S):
        c = scale * (i + 0.5)
        lo, hi = max(0, math.floor(c - support + 0.5)), min(side, math.floor(c + support + 0.5))
        j = torch.arange(lo, hi, dtype=torch.float64)
        w = (1.0 - ((j - c + 0.5) * inv).abs()).clamp_min(0.0)
        Wm[i, lo:hi] = w / w.sum()
        taps = max(taps, hi - lo)
    return Wm, taps


def aa_weights_integer(side, S):
    """The same weights from integers alone (what the kernel does): n(i, j) = max(0, D - |(2 j + 1) S - side (2 i + 1)|), D = 2 max(side, S),
    window bounds by floor division."""
    D = 2 * max(side, S)
    Wm = torch.zeros(S, side, dtype=torch.float64)
    for i in range(S):
        c2 = side * (2 * i + 1)
        lo, hi = max(0, (c2 - D + S) // (2 * S)), min(side, (c2 + D + S) // (2 * S))
        n = [max(0, D - abs((2 * j + 1) * S - c2)) for j in range(lo, hi)]
        Wm[i, lo:hi] = torch.tensor(n, dtype=torch.float64) / sum(n)
    return Wm


def resize(crop_u8, S, dtype=torch.float64):
    """[3, S, S] of a [side, side, 3] uint8 crop: / 255, then the antialiased resize on both axes, in ``dtype``; also (tx, ty)."""
    side = crop_u8.shape[0]
    Wm, taps = aa_weights(side, S)
    Wm = Wm.to(dtype)
    x = torch.from_numpy(np.ascontiguousarray(crop_u8)).permute(2, 0, 1).to(dtype) / 255
    return Wm @ x @ Wm.t(), (taps, taps)


def resize_bound(tx, ty):
    """fp32 accumulation of a convex combination of values in [0, 1]: one rounding per tap, six more for the weights, the hand-over
    between the axes and the division; the factor 2 is margin."""
    return 2 * (tx + ty + 6) * EPS24


# ---- colour -------------------------------------------------------------------------------------------------------------------------
def grey(x):
    return 0.2989 * x[0] + 0.587 * x[1] + 0.114 * x[2]


def _rgb2hsv(img):
    r, g, b = img.unbind(0)
    maxc, minc = img.max(0).values, img.min(0).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    return torch.stack((h, s, maxc))


def _hsv2rgb(img):
    h, s, v = img.unbind(0)
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int32) % 6
    p = (v * (1.0 - s)).clamp(0.0, 1.0)
    q = (v * (1.0 - s * f)).clamp(0.0, 1.0)
    t = (v * (1.0 - s * (1.0 - f))).clamp(0.0, 1.0)
    mask = i.unsqueeze(0) == torch.arange(6, device=img.device).view(-1, 1, 1)
    a1, a2, a3 = torch.stack((v, q, p, p, t, v)), torch.stack((t, v, v, q, p, p)), torch.stack((p, p, t, v, v, q))
    a4 = torch.stack((a1, a2, a3))
    return torch.einsum("ijk,xijk->xjk", mask.to(img.dtype), a4)


def colour_op(x, op, e):
    if op == 0:
        return (e["brightness"] * x).clamp(0.0, 1.0)
    if op == 1:
        return (e["contrast"] * x + (1.0 - e["contrast"]) * grey(x).mean()).clamp(0.0, 1.0)
    if op == 2:
        return (e["saturation"] * x + (1.0 - e["saturation"]) * grey(x)).clamp(0.0, 1.0)
    hsv = _rgb2hsv(x)
    hsv = torch.stack((torch.remainder(hsv[0] + e["hue"], 1.0), hsv[1], hsv[2]))
    return _hsv2rgb(hsv)


def apply_colour(x, e):
    """The colour stage on one resized frame [3, S, S] in its own dtype; ``e``: a dict as posediffusion_amd.images.draw_colour returns."""
    if e is None:
        return x
    if e.get("jitter"):
        for op in e["order"]:
            x = colour_op(x, int(op), e)
    if e.get("grayscale"):
        x = grey(x).unsqueeze(0).expand(3, -1, -1).clone()
    top, left, h, w = e.get("erase") or (0, 0, 0, 0)
    if h:
        x = x.clone()
        x[:, top:top + h, left:left + w] = 0
    return x


def yardstick(img, box, S, fill=0, colour=None, dtype=torch.float64):
    """One frame through the whole path in ``dtype``: (out [3, S, S], (tx, ty)).  ``box`` = (x0, y0, side)."""
    x, taps = resize(padded_crop(img, box[0], box[1], box[2], fill), S, dtype)
    if colour is not None:      # the factors as the kernel receives them: fp32 values
        colour = dict(colour, **{k: float(np.float32(colour[k])) for k in ("brightness", "contrast", "saturation", "hue") if k in colour})
    return apply_colour(x, colour), taps


# ---- case tables ----------------------------------------------------------------------------------------------------------------------
def picture(h, w, seed):
    """A picture with smooth ramps, hard edges and noise, so that every filter tap matters."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack(((xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx // 7 + yy // 5) % 2) * 255), axis=-1).astype(np.int64)
    img = np.clip(img + rng.integers(-40, 41, size=img.shape), 0, 255)
    return img.astype(np.uint8)


def palette(side):
    """Exact greys, black, white, saturated primaries and their mixes in blocks, the rest noise (read with side == S: no blending)."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(side, side, 3)).astype(np.uint8)
    cols = [(0, 0, 0), (255, 255, 255), (128, 128, 128), (37, 37, 37), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255),
            (255, 0, 255), (200, 200, 10), (10, 200, 200), (1, 0, 0), (254, 255, 255), (90, 90, 91), (255, 128, 0)]
    for k, c in enumerate(cols):
        img[2 * (k // 4):2 * (k // 4) + 2, 4 * (k % 4):4 * (k % 4) + 4] = c
    return img


# (name, H, W, (x0, y0, side)); S = 32, every one of them with fill 0 and the border ones with fill 255 as well
SQUARE_SIDES = (32, 33, 31, 64, 97, 320, 1280, 5, 1)
RESIZE_CASES = [(f"side{s}", s, s, (0, 0, s)) for s in SQUARE_SIDES]
BORDER_CASES = [("left", 80, 100, (-10, 20, 40)), ("top", 80, 100, (30, -15, 40)), ("right", 80, 100, (75, 20, 40)),
                ("bottom", 80, 100, (30, 60, 40)), ("all_four", 80, 100, (-20, -30, 150)), ("outside_far", 80, 100, (200, 200, 40)),
                ("outside_neg", 80, 100, (-100, -100, 40)), ("odd_rows", 53, 37, (0, 5, 37)), ("odd_rows_over", 53, 37, (-3, 10, 43))]
ALL_CASES = RESIZE_CASES + BORDER_CASES


def case_picture(name, H, W):
    return picture(H, W, seed=sum(map(ord, name)))


# the reference's ColorJitter ranges: brightness, contrast in [0.6, 1.4], saturation in [0.8, 1.2], hue in [-0.1, 0.1]
FACTOR_SETS = ((0.6, 0.6, 0.8, -0.1), (1.4, 1.4, 1.2, 0.1), (0.6, 1.4, 0.8, 0.1), (1.13, 0.87, 1.07, 0.031))
ORDERS = tuple(itertools.permutations(range(4)))


def colour_table():
    return [dict(jitter=1, order=o, brightness=f[0], contrast=f[1], saturation=f[2], hue=f[3], grayscale=0, erase=(0, 0, 0, 0))
            for o in ORDERS for f in FACTOR_SETS]


def colour_sources():
    """The two source frames of the colour table: exact colours read without blending, and a busy picture reduced 97 -> 32."""
    return [(palette(32), (0, 0, 32)), (picture(97, 97, seed=97), (0, 0, 97))]


def own_error_bound(cases, S=32, margin=4):
    """``margin`` x the largest distance of an fp32 run of the yardstick from the fp64 yardstick over ``cases`` = (img, box, colour) (the
    project's convention for fp32-grade kernels, tests/test_gpu_vit_tokens.py); also the fp64 results, in order."""
    worst, refs = 0.0, []
    for img, box, e in cases:
        r64, _ = yardstick(img, box, S, colour=e)
        r32, _ = yardstick(img, box, S, colour=e, dtype=torch.float32)
        worst = max(worst, (r32.double() - r64).abs().max().item())
        refs.append(r64)
    return margin * worst, refs


def colour_table_bound():
    return own_error_bound([(img, box, e) for img, box in colour_sources() for e in colour_table()])


# ---- a Co3D tree in miniature ---------------------------------------------------------------------------------------------------------------
def write_co3d_tree(root, n_frames=6, sizes=((60, 90), (75, 50))):
    """A Co3D tree in miniature: PNG frames of two sizes, one good sequence per size, one too short, one with a ridiculous translation."""
    rng = np.random.default_rng(11)
    ann = {}
    for s, (h, w) in enumerate(sizes):
        seq = []
        for k in range(n_frames):
            rel = os.path.join("apple", f"seq{s}", "images", f"frame{k:03d}.png")
            os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
            Image.fromarray(picture(h, w, seed=10 * s + k)).save(os.path.join(root, rel))
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            q = q * np.sign(np.linalg.det(q))
            seq.append({"filepath": rel, "bbox": [5, 7, w - 9, h - 4], "R": q.tolist(), "T": (rng.normal(size=3) + [0, 0, 4]).tolist(),
                        "focal_length": rng.uniform(1.5, 3.0, 2).tolist(), "principal_point": rng.uniform(-0.1, 0.1, 2).tolist(),
                        "unused": 1})
        ann[f"seq{s}"] = seq
    ann["short"] = [dict(ann["seq0"][0]) for _ in range(2)]
    ann["far"] = [dict(d, T=[1e5, 1.0, 1.0]) for d in ann["seq0"]]
    os.makedirs(os.path.join(root, "anno"), exist_ok=True)
    with gzip.open(os.path.join(root, "anno", "apple_train.jgz"), "w") as fh:
        fh.write(json.dumps(ann).encode())
    return dict(category=("apple",), split="train", min_num_images=4, img_size=32, CO3D_DIR=root, CO3D_ANNOTATION_DIR=os.path.join(root, "anno"))
