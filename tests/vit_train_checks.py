"""Gradient yardstick for the backbone trainer (include/pd_engine_vit_train.h): ``multiscale`` restates
oracle/vit_oracle.multiscale_features WITH grad (the oracle's is ``no_grad``; the arithmetic is the same line for line, so the forward is
the oracle's bit for bit), and ``reference`` differentiates S = sum(g_z * z) with torch.autograd in float64 (the yardstick) and in
float32 ("own": what torch itself is away from float64 on the same function).  Every operation of the ViT is smooth -- GELU, softmax,
LayerNorm -- so no teacher forcing is needed, unlike tests/train_checks.py.

Shared by tests/test_vit_train_checks_cpu.py and tests/test_gpu_vit_train.py; ``grad_dist`` is train_checks'."""
from __future__ import annotations

import copy
import math
from typing import Dict, NamedTuple, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import vit_oracle as VO
from train_checks import grad_dist  # noqa: F401  (re-exported)

FLOOR = 8 * 2.0 ** -24            # four fp32 ulps of a tensor's largest entry (an ulp of a value in [1, 2) is 2^-23 = 2 x 2^-24): own is exactly 0 for
                                  # norm.bias at one image, where the gradient is g_z itself, and no fp32 kernel chain can be asked to be exact there
MARGIN = 4.0


def bound(own: float, margin: float = MARGIN) -> float:
    """The distance from float64 a tensor may have: margin x own, at least FLOOR."""
    return max(margin * own, FLOOR)


def multiscale(net: nn.Module, image_rgb: torch.Tensor, scale_factors=(1, 1 / 2, 1 / 3)) -> torch.Tensor:
    """vit_oracle.multiscale_features without ``no_grad`` (models/image_feature_extractor.py:57-87)."""
    mean = torch.tensor(VO.RESNET_MEAN, dtype=image_rgb.dtype).view(1, 3, 1, 1)
    std = torch.tensor(VO.RESNET_STD, dtype=image_rgb.dtype).view(1, 3, 1, 1)
    img = (image_rgb - mean) / std
    feats = None
    for sf in scale_factors:
        inp = img if sf == 1 else F.interpolate(img, scale_factor=sf, mode="bilinear", align_corners=False)
        f = net(inp)
        feats = f if feats is None else feats + f
    return feats / len(scale_factors)


def make_net(depth: int, seed: int = 0) -> VO.DinoViT:
    """vit_oracle.make_vit cut to its first ``depth`` blocks (float32), with a non-trivial cls_token / pos_embed scale left as drawn."""
    net = VO.make_vit(seed=seed)
    net.blocks = nn.ModuleList(list(net.blocks)[:depth])
    return net


class Case(NamedTuple):
    n: int
    H: int
    W: int
    scales: Tuple[float, ...]
    depth: int

    @property
    def label(self) -> str:
        return f"n{self.n}_{self.H}x{self.W}_s{len(self.scales)}_d{self.depth}"


THREE = (1, 1 / 2, 1 / 3)


def inputs(case: Case, seed: int = 0):
    """(images [n, 3, H, W] in [0, 1), g_z [n, 384]) of a case, from a seed."""
    g = torch.Generator().manual_seed(4100 + 7 * case.n + case.H + 3 * case.W + seed)
    return torch.rand(case.n, 3, case.H, case.W, generator=g), torch.randn(case.n, 384, generator=g)


class _BicubicOntoItself(torch.autograd.Function):
    """F.interpolate(x [1, C, g, g], scale_factor, bicubic) onto the SAME size, with the adjoint of its own forward.  torch's CPU forward
    evaluates the scale factor there (DINO's (g + 0.1) / g moves source coordinates by up to 0.1 cell), but its backward copies the
    gradient whenever input and output sizes are equal: autograd then returns a pos_embed gradient that is not the derivative of the
    forward (tests/test_vit_train_edges_cpu.py holds both against finite differences).  The map is linear, so its matrix is read off the
    forward itself -- the identity basis pushed through it -- and the backward is that matrix transposed: no restated arithmetic."""

    @staticmethod
    def forward(ctx, x, scale_factor):
        ctx.scale_factor, ctx.shape = scale_factor, x.shape
        return F.interpolate(x, scale_factor=scale_factor, mode="bicubic")

    @staticmethod
    def backward(ctx, gy):
        _, C, ga, gb = ctx.shape
        basis = torch.eye(ga * gb, dtype=gy.dtype).reshape(ga * gb, 1, ga, gb)
        K = F.interpolate(basis, scale_factor=ctx.scale_factor, mode="bicubic").reshape(ga * gb, -1)      # [input cell, output cell]
        return (gy.reshape(C, -1) @ K.T).reshape(ctx.shape), None


def _differentiable_pos_encoding(m: nn.Module):
    """``m.interpolate_pos_encoding`` for autograd: DINO's own lines (oracle/vit_oracle.py:96-109, the same values bit for bit), with
    `_BicubicOntoItself` where the trained grid is resampled onto its own size -- the one branch in which torch's backward is not the
    forward's adjoint.  Every other input takes the oracle's method itself."""
    dino = m.interpolate_pos_encoding

    def rule(x, w, h):
        N = m.pos_embed.shape[1] - 1
        if x.shape[1] - 1 != N or w == h:
            return dino(x, w, h)
        dim, g, p = x.shape[-1], int(math.sqrt(N)), m.patch_embed.patch_size
        w0, h0 = w // p + 0.1, h // p + 0.1
        assert (w // p, h // p) == (g, g)
        pp = _BicubicOntoItself.apply(m.pos_embed[:, 1:].reshape(1, g, g, dim).permute(0, 3, 1, 2), (w0 / g, h0 / g))
        return torch.cat((m.pos_embed[:, 0].unsqueeze(0), pp.permute(0, 2, 3, 1).reshape(1, -1, dim)), dim=1)
    return rule


def reference(net: nn.Module, images: torch.Tensor, g_z: torch.Tensor, scale_factors, dtype) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """(z, {state-dict name: dS/d param}) of S = sum(g_z * z) in ``dtype`` on the CPU, from a copy of ``net``."""
    m = copy.deepcopy(net).to(dtype)
    m.interpolate_pos_encoding = _differentiable_pos_encoding(m)
    for p in m.parameters():
        p.requires_grad_(True)
    z = multiscale(m, images.to(dtype), scale_factors)
    names = [n for n, _ in m.named_parameters()]
    gs = torch.autograd.grad((z * g_z.to(dtype)).sum(), [p for _, p in m.named_parameters()], allow_unused=True)
    params = dict(m.named_parameters())
    return z.detach(), {n: (torch.zeros_like(params[n]) if g is None else g.detach()) for n, g in zip(names, gs)}


def image_contribution(net: nn.Module, images: torch.Tensor, g_z: torch.Tensor, scale_factors, image: int, dtype=torch.float64):
    """The part of `reference`'s gradients that ONE image carries: S is linear in g_z, so it is the reference with g_z zero elsewhere."""
    only = torch.zeros_like(g_z)
    only[image] = g_z[image]
    return reference(net, images, only, scale_factors, dtype)[1]


def z_on_unresampled_table(net: nn.Module, images: torch.Tensor, scale_factors, dtype=torch.float64) -> torch.Tensor:
    """z of a copy of ``net`` that takes ``pos_embed`` as it stands whenever the token grid is the trained one, whatever the pixel sizes:
    the rule DINO does NOT have (its copy branch also asks for equal height and width).  For inputs DINO resamples this is a wrong z."""
    m = copy.deepcopy(net).to(dtype)
    dino = m.interpolate_pos_encoding

    def rule(x, w, h):
        return m.pos_embed if x.shape[1] == m.pos_embed.shape[1] else dino(x, w, h)
    m.interpolate_pos_encoding = rule
    with torch.no_grad():
        return multiscale(m, images.to(dtype), scale_factors)


def with_row_stride(images: torch.Tensor, stride: int) -> torch.Tensor:
    """[n, 3, H, stride] read out of the pixel buffer of ``images`` [n, 3, H, W] (stride <= W) with ``stride`` as the row stride of every
    channel plane: what a kernel sees that steps rows by 16 x (W // 16) instead of W."""
    n, c, H, W = images.shape
    assert stride <= W
    return images.contiguous().as_strided((n, c, H, stride), (c * H * W, H * W, stride, 1)).clone()


def vt_chunks(M: int, max_chunks: int = 16) -> Tuple[int, int, int]:
    """(chunks, rows per chunk, rows of the last chunk) of a reduction over M token rows: pd_tr_chunks of
    posediffusion_amd/csrc/pd_train_launch.h restated (``max_chunks`` = PD_TR_MAX_CHUNKS); tests/test_vit_train_edges_cpu.py compiles that
    header and holds the two against each other."""
    n = min(max_chunks, (M + 255) // 256)
    r = (M + n - 1) // n
    r = (r + 31) // 32 * 32
    chunks = (M + r - 1) // r
    return chunks, r, M - (chunks - 1) * r


def grad_blocks(name: str, g: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The sub-blocks of a gradient whose magnitudes differ so much that a whole-tensor maximum would hide one of them: the q, k and v
    rows of ``attn.qkv.weight`` / ``attn.qkv.bias`` (v from P^T dO dominates), and row 0 (the CLS position, about 10 x the rest: every
    image's CLS token feeds z directly) against rows 1 .. of ``pos_embed``.  {} for every other tensor."""
    if name.endswith(("attn.qkv.weight", "attn.qkv.bias")):
        d = g.shape[0] // 3
        return {"q": g[:d], "k": g[d:2 * d], "v": g[2 * d:]}
    if name == "pos_embed":
        g = g.reshape(-1, g.shape[-1])
        return {"cls": g[:1], "patch": g[1:]}
    return {}


def block_dists(name: str, g, g_own, g64):
    """[(block, distance of g, distance of g_own, zero)] per block of `grad_blocks`, each against that block's OWN float64 maximum."""
    b, bo, b64 = (grad_blocks(name, torch.as_tensor(t).detach().cpu()) for t in (g, g_own, g64))
    return [(k, grad_dist(b[k], b64[k]), grad_dist(bo[k], b64[k]), b64[k].abs().max().item() == 0.0) for k in b64]


def is_k_bias(name: str, block: str) -> bool:
    """The k rows of ``attn.qkv.bias``: a key bias shifts every score of a softmax row equally, so their gradient is mathematically zero
    and float64 holds only its own rounding there -- printed, never asserted (as train_checks.block_misses does for in_proj_bias)."""
    return block == "k" and name.endswith("attn.qkv.bias")


def worst_ratio(z, grads, ref64, ref32) -> Tuple[float, str]:
    """(distance / bound, label) of whichever of z, the gradient tensors and their asserted blocks uses most of its bound (at the plain
    margin of 4): the figure profiles/vit_train_parity.txt records per case.  Blocks that are zero in float64 are left out."""
    (z64, g64), (z32, g32) = ref64, ref32
    rows = [("z", grad_dist(z, z64), grad_dist(z32, z64), False)]
    for name in g64:
        rows.append((name, grad_dist(grads[name], g64[name]), grad_dist(g32[name], g64[name]), g64[name].abs().max().item() == 0.0))
        rows += [(f"{name}[{k}]", e, own, zero) for k, e, own, zero in block_dists(name, grads[name], g32[name], g64[name]) if not is_k_bias(name, k)]
    return max((e / bound(own), lab) for lab, e, own, zero in rows if not zero)


def misses(name: str, g, g_own, g64, margins=None):
    """[(label, distance, own)] of the tensor and of each of its blocks that is further from float64 than `bound` allows (``margins``:
    {label: recorded margin}), or that is not exactly zero where float64's is identically zero."""
    margins = margins or {}
    rows = [(name, grad_dist(g, g64), grad_dist(g_own, g64), torch.as_tensor(g64).abs().max().item() == 0.0)]
    rows += [(f"{name}[{k}]", e, own, zero) for k, e, own, zero in block_dists(name, g, g_own, g64) if not is_k_bias(name, k)]
    return [(lab, e, own) for lab, e, own, zero in rows if (zero and e != 0.0) or (not zero and e > bound(own, margins.get(lab, MARGIN)))]
