"""Yardstick of the trainer's dropout (pd_train_forward_dropout, include/pd_engine_train.h; DESIGN 3.9 "Dropout"): the host mirror of the
mask definition, and train_checks' teacher-forced float64 / float32 p_losses with the four dropout sites of every encoder layer applied
from that mirror.  Written from the definition in the header, not from the kernels.

The mask.  For a call with (seed: uint64, step: uint32, p) the element at (row r, column c) of site s of encoder layer l is KEPT iff word
r & 3 of  philox4x32_10(counter = (r >> 2, c, 4 l + s, step), key = (seed & 0xffffffff, seed >> 32))  is >= thr = floor(p 2^32); kept values
are multiplied by scale = 1 / (1 - p).  p crosses the C-ABI as a float, so thr and scale are those of float32(p): thr is computed in double
from it, scale is the fp32 quotient.  Sites (nn.TransformerEncoderLayer's, in this order):
  0 attention probabilities, row (b nhead + h) N + i, column = key j      1 dropout1 on out_proj(ctx) + bias, row = token row m
  2 the FF dropout after linear1's ReLU, row m, column < dim_ff           3 dropout2 on linear2(..) + bias, row m
Shared by tests/test_train_dropout_cpu.py, tests/test_gpu_train_dropout.py and tests/perf/train_dropout_bench.py."""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch

from oracle import pd_oracle as O
import train_checks as TC

ATTN, RESID1, FF, RESID2, ALL = 1, 2, 4, 8, 15
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., Random123): ``counter`` = four and ``key`` = two broadcastable integer arrays of 32-bit words ->
    the four output words as uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK32]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def threshold(p: float) -> int:
    """thr = (uint32) floor(p 2^32), in double, of the float the ABI carries."""
    return int(math.floor(float(np.float32(p)) * 4294967296.0))


def scale_of(p: float) -> float:
    """1 / (1 - p) as the fp32 value the host computes once."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(rows: int, cols: int, layer: int, site: int, seed: int, step: int, p: float) -> np.ndarray:
    """[rows, cols] bool: True where the element is kept."""
    seed = int(seed) % 2 ** 64
    r, c = np.arange(rows, dtype=np.uint64)[:, None], np.arange(cols, dtype=np.uint64)[None, :]
    words = philox4x32_10((r >> np.uint64(2), c, 4 * layer + site, int(step)), (seed & 0xFFFFFFFF, seed >> 32))
    sel = (r & np.uint64(3)) + np.zeros_like(c)
    word = np.choose(sel.astype(np.int64), words)
    return word >= np.uint32(threshold(p))                     # p < 1: the threshold fits 32 bits


def _keep(shape_rows: int, cols: int, layer: int, site: int, drop, dtype) -> torch.Tensor:
    p, seed, step = drop
    return torch.from_numpy(keep_mask(shape_rows, cols, layer, site, seed, step, p)).to(dtype) * scale_of(p)


def attention(sd: Dict[str, torch.Tensor], prefix: str, a: torch.Tensor, nhead: int, layer: int, sites: int, drop, pmax=None) -> torch.Tensor:
    """Self-attention of the rows ``a`` [B, N, d] through out_proj (+ bias), with site 0 on the probabilities when ``sites`` has it."""
    B, N, d = a.shape
    dh = d // nhead
    qkv = a @ sd[prefix + "self_attn.in_proj_weight"].T + sd[prefix + "self_attn.in_proj_bias"]
    q, k, v = (u.reshape(B, N, nhead, dh).transpose(1, 2) for u in qkv.split(d, dim=-1))
    att = torch.softmax((q / math.sqrt(dh)) @ k.transpose(-1, -2), dim=-1)
    if pmax is not None:
        pmax.append(att.detach().max(dim=-1).values)
    if sites & ATTN:
        att = att * _keep(B * nhead * N, N, layer, 0, drop, a.dtype).reshape(B, nhead, N, N)
    ctx = (att @ v).transpose(1, 2).reshape(B, N, d)
    return ctx @ sd[prefix + "self_attn.out_proj.weight"].T + sd[prefix + "self_attn.out_proj.bias"]


def encoder_layer(sd: Dict[str, torch.Tensor], prefix: str, h: torch.Tensor, nhead: int, layer: int, sites: int, drop, relu_mask=None,
                  pre=None, used=None, pmax=None) -> torch.Tensor:
    """One pre-norm encoder layer of train_checks.denoiser_forward (h: [B, N, d]) with dropout ``drop`` = (p, seed, step) at ``sites``;
    a site that is off leaves the arithmetic of train_checks untouched."""
    B, N, d = h.shape
    pre, used = ([] if pre is None else pre), ([] if used is None else used)
    o = attention(sd, prefix, O._layer_norm(h, sd[prefix + "norm1.weight"], sd[prefix + "norm1.bias"]), nhead, layer, sites, drop, pmax)
    if sites & RESID1:
        o = o * _keep(B * N, d, layer, 1, drop, h.dtype).reshape(B, N, d)
    h = h + o
    a = O._layer_norm(h, sd[prefix + "norm2.weight"], sd[prefix + "norm2.bias"])
    a = TC._relu(a @ sd[prefix + "linear1.weight"].T + sd[prefix + "linear1.bias"], relu_mask, pre, used)
    if sites & FF:
        a = a * _keep(B * N, a.shape[-1], layer, 2, drop, h.dtype).reshape(a.shape)
    o = a @ sd[prefix + "linear2.weight"].T + sd[prefix + "linear2.bias"]
    if sites & RESID2:
        o = o * _keep(B * N, d, layer, 3, drop, h.dtype).reshape(B, N, d)
    return h + o


def denoiser_forward_dropout(sd, net: TC.Net, x, t, z, sites: int, drop, masks=None):
    """train_checks.denoiser_forward with the encoder layers' dropout; same return value (info["pre"] are the ReLU inputs, before any mask)."""
    B, N, _ = x.shape
    pre, used, pmax = [], [], []
    t_emb = O.timestep_embedding(t, sd)[:, None, :].expand(-1, N, -1)
    parts = [O.harmonic_embedding(x), t_emb, z]
    if net.pivot:
        pivot = torch.zeros_like(z[..., :1])
        pivot[:, 0] = 1.0
        parts.append(pivot)
    h = torch.cat(parts, dim=-1) @ sd["_first.weight"].T + sd["_first.bias"]
    for l in range(net.layers):
        h = encoder_layer(sd, f"_trunk.layers.{l}.", h, net.nhead, l, sites, drop, None if masks is None else masks[l], pre, used, pmax)
    a = O._layer_norm(h @ sd["_last.0.weight"].T + sd["_last.0.bias"], sd["_last.1.weight"], sd["_last.1.bias"])
    a = TC._relu(a, None if masks is None else masks[net.layers], pre, used)
    return a @ sd["_last.3.weight"].T + sd["_last.3.bias"], {"pre": pre, "masks": used, "pmax": pmax}


def loss_and_grads_dropout(sd, net: TC.Net, inp, objective: str, loss_type: str, p: float, sites: int, seed: int, step: int, g_loss=None,
                           masks=None, signs=None, dtype=torch.float64, want=None):
    """train_checks.loss_and_grads of the function with dropout: same arguments, same result dict.  ``masks`` force the ReLUs as there
    (the engine's "ReLU passed and kept" masks are a subset of the kept elements, so forcing them and applying keep_mask agree)."""
    if p == 0.0:
        sites = 0
    sd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    tables = O.diffusion_tables(dtype=dtype)
    x_start, noise, t = inp["x_start"].to(dtype), inp["noise"].to(dtype), inp["t"]
    z = inp["z"].detach().to(dtype).requires_grad_(True)
    x_t = TC.q_sample(x_start, noise, t, tables)
    out, info = denoiser_forward_dropout(sd, net, x_t, t, z, sites, (p, seed, step), masks)
    target = noise if objective == "pred_noise" else x_start
    d = out - target
    if loss_type == "l1":
        s = torch.sign(d.detach()) if signs is None else signs.to(dtype).reshape(d.shape)
        loss = d * s
    else:
        s = torch.sign(d.detach())
        loss = d * d
    g = torch.full_like(loss, 1.0 / loss.numel()) if g_loss is None else g_loss.to(dtype).reshape(loss.shape)
    names = list(sd) if want is None else [n for n in want if n != "z"]
    gs = torch.autograd.grad((g * loss).sum(), [sd[n] for n in names] + [z], allow_unused=True)
    grads = {n: (torch.zeros_like(sd[n]) if v is None else v) for n, v in zip(names, gs[:-1])}
    grads["z"] = gs[-1]
    return {"loss": loss.detach(), "model_out": out.detach(), "x_t": x_t, "target": target, "grads": grads, "pre": info["pre"],
            "masks": info["masks"], "signs": s}


def site_shapes(B: int, N: int, nhead: int, d_model: int, dim_ff: int):
    """(rows, cols) of the four sites' masks at (B, N)."""
    return [(B * nhead * N, N), (B * N, d_model), (B * N, dim_ff), (B * N, d_model)]


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gpu_train_dropout.py
# (name, configuration, B, N, p, sites, seed, step, objective, loss_type); configuration: "two" = the default network with 2 encoder
# layers, "small" = d 96 / head dim 24 / ff 200 / no pivot with 2 layers, "default" = the 8-layer default.  test_train_dropout_cpu.py
# checks every mask of every case against the binomial bound on the CPU: the masks are deterministic, so the seeds are chosen there.
CONFIGS = {"two": (512, 4, 1024, 2), "small": (96, 4, 200, 2), "default": (512, 4, 1024, 8)}       # d_model, nhead, dim_ff, layers
GPU_CASES = (
    [(f"site{s}_p{p}", "two", 3, 5, p, s, 11, 0, "pred_noise", "l1") for s in (ATTN, RESID1, FF, RESID2, ALL) for p in (0.1, 0.5)]
    + [("n1", "two", 1, 1, 0.5, ALL, 12, 0, "pred_noise", "l1"),
       ("b2n64", "two", 2, 64, 0.1, ALL, 13, 0, "pred_noise", "l1"),
       ("b2n63", "two", 2, 63, 0.1, ALL, 14, 0, "pred_noise", "l1"),
       ("b7n19", "two", 7, 19, 0.1, ALL, 15, 3, "pred_noise", "l1"),
       ("small_b3n7", "small", 3, 7, 0.1, ALL, 16, 0, "pred_noise", "l1"),
       ("default_b3n5", "default", 3, 5, 0.1, ALL, 17, 0, "pred_noise", "l1"),
       ("m257", "small", 257, 1, 0.1, ALL, 18, 0, "pred_noise", "l1"),
       ("x0_l2", "two", 3, 5, 0.1, ALL, 19, 0, "pred_x0", "l2"),
       ("noise_l2", "two", 3, 5, 0.1, ALL, 20, 0, "pred_noise", "l2"),
       ("x0_l1", "two", 3, 5, 0.1, ALL, 21, 0, "pred_x0", "l1")])
