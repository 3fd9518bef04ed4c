"""Yardstick of the trainer's key-tiled attention (pd_tr_lattn_* kernels, posediffusion_amd/csrc/pd_train_lattn.h; DESIGN 3.9 "65 ... 256
frames"): a float64 torch mirror of the two-phase tiled scheme, written from DESIGN's description and not from the kernels, and the cases
of tests/test_gpu_train_long.py (their dropout masks are checked on the CPU in tests/test_train_long_cpu.py).

The scheme, per (sequence, head), keys in tiles of TILE = 64, query rows in blocks of ROWS = 16:
  forward   s = (scale q) k^T tile by tile; mx = max over all scores; e = exp(s - mx); sum = sum over the lanes of (e0 + e1 + e2 + e3);
            p = e (1 / sum); with dropout p~ = keep ? p ks : 0 (ks = 1 / (1 - p_drop)); ctx = sum over the tiles, ascending, of p~ v.
  phase A   dP = dO v^T tile by tile; with dropout dP = keep ? dP ks : 0 (a select); rs = sum(dP P of tile 0) + sum(dP P of tiles 1 ..);
            dS = P (dP - rs) with the UNMASKED P; dQ = scale sum over the tiles, ascending, of dS k; (mx, 1 / sum, rs) are kept per row.
  phase B   per key tile, the query blocks in ascending order: P, P~, dP, dS of the block recomputed from (mx, 1 / sum, rs) by the same
            expressions; dV += P~^T dO, dK += dS^T q (unscaled q), dK times scale at the end.
Shared by tests/test_train_long_cpu.py, tests/test_gpu_train_long.py and tests/perf/train_long_bench.py."""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

from oracle import pd_oracle as O
import train_checks as TC
import train_dropout_checks as D

TILE, ROWS, MAX_FRAMES = 64, 16, 256


def _tiles(N: int):
    return [(j0, min(N, j0 + TILE)) for j0 in range(0, N, TILE)]


def tiled_forward(q, k, v, scale: float, keep: Optional[torch.Tensor] = None, ks: float = 1.0):
    """q, k, v: [N, hd] float64 of one (sequence, head); keep: [N, N] bool or None.  -> (ctx [N, hd], stats [N, 3] = (mx, 1 / sum, 0))."""
    N, hd = q.shape
    ctx, stats = torch.zeros(N, hd, dtype=q.dtype), torch.zeros(N, 3, dtype=q.dtype)
    for i0 in range(0, N, ROWS):
        qs = q[i0:i0 + ROWS] * scale
        s = [qs @ k[a:b].T for a, b in _tiles(N)]
        mx = torch.stack([t.max(dim=1).values for t in s]).max(dim=0).values
        e = [torch.exp(t - mx[:, None]) for t in s]
        lane = torch.zeros(qs.shape[0], TILE, dtype=q.dtype)          # per lane e0 + e1 + e2 + e3, then the sum over the lanes
        for t in e:
            lane[:, :t.shape[1]] += t
        inv = 1.0 / lane.sum(dim=1)
        acc = torch.zeros(qs.shape[0], hd, dtype=q.dtype)
        for (a, b), t in zip(_tiles(N), e):
            p = t * inv[:, None]
            if keep is not None:
                p = torch.where(keep[i0:i0 + ROWS, a:b], p * ks, torch.zeros_like(p))
            acc = acc + p @ v[a:b]
        ctx[i0:i0 + ROWS] = acc
        stats[i0:i0 + ROWS, 0], stats[i0:i0 + ROWS, 1] = mx, inv
    return ctx, stats


def _block(qs, k_t, v_t, dO_b, mx, inv, keep_b, ks):
    """(P, P~, dP) of one [rows x tile] block from the row statistics: THE expressions both phases use."""
    p = torch.exp(qs @ k_t.T - mx[:, None]) * inv[:, None]
    dp = dO_b @ v_t.T
    pt = p
    if keep_b is not None:
        dp = torch.where(keep_b, dp * ks, torch.zeros_like(dp))
        pt = torch.where(keep_b, p * ks, torch.zeros_like(p))
    return p, pt, dp


def tiled_backward(q, k, v, dO, scale: float, stats, keep: Optional[torch.Tensor] = None, ks: float = 1.0):
    """-> (dq, dk, dv), each [N, hd]; ``stats`` from tiled_forward (its third column is filled with rs by phase A)."""
    N, hd = q.shape
    dq, dk, dv = (torch.zeros(N, hd, dtype=q.dtype) for _ in range(3))
    stats = stats.clone()
    tiles = _tiles(N)
    for i0 in range(0, N, ROWS):                                      # phase A
        rows = slice(i0, min(N, i0 + ROWS))
        qs, mx, inv = q[rows] * scale, stats[rows, 0], stats[rows, 1]
        blocks = [_block(qs, k[a:b], v[a:b], dO[rows], mx, inv, None if keep is None else keep[rows, a:b], ks) for a, b in tiles]
        rs = (blocks[0][2] * blocks[0][0]).sum(dim=1)
        if len(blocks) > 1:
            lane = torch.zeros(qs.shape[0], TILE, dtype=q.dtype)
            for p, _, dp in blocks[1:]:
                lane[:, :p.shape[1]] += dp * p
            rs = rs + lane.sum(dim=1)
        acc = torch.zeros(qs.shape[0], hd, dtype=q.dtype)
        for (a, b), (p, _, dp) in zip(tiles, blocks):
            acc = acc + (p * (dp - rs[:, None])) @ k[a:b]
        dq[rows] = scale * acc
        stats[rows, 2] = rs
    for a, b in tiles:                                                # phase B
        acc_k, acc_v = torch.zeros(b - a, hd, dtype=q.dtype), torch.zeros(b - a, hd, dtype=q.dtype)
        for i0 in range(0, N, ROWS):
            rows = slice(i0, min(N, i0 + ROWS))
            p, pt, dp = _block(q[rows] * scale, k[a:b], v[a:b], dO[rows], stats[rows, 0], stats[rows, 1],
                               None if keep is None else keep[rows, a:b], ks)
            ds = p * (dp - stats[rows, 2][:, None])
            acc_v = acc_v + pt.T @ dO[rows]
            acc_k = acc_k + ds.T @ q[rows]
        dk[a:b], dv[a:b] = scale * acc_k, acc_v
    return dq, dk, dv


def plain_attention_grads(q, k, v, dO, scale: float, keep: Optional[torch.Tensor] = None, ks: float = 1.0):
    """autograd of softmax((scale q) k^T) (x keep ks) v against the cotangent dO -> (ctx, dq, dk, dv)."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    att = torch.softmax((q * scale) @ k.T, dim=-1)
    if keep is not None:
        att = att * (keep.to(q.dtype) * ks)
    ctx = att @ v
    dq, dk, dv = torch.autograd.grad((ctx * dO).sum(), [q, k, v])
    return ctx.detach(), dq, dk, dv


def _log_probs(sd, net: TC.Net, x, t, z) -> List[torch.Tensor]:
    """log of the softmax rows [B, nhead, N, N] of every encoder layer of train_checks.denoiser_forward (no dropout, own masks), in the
    dtype of the arguments and differentiable with respect to them"""
    B, N, _ = x.shape
    parts = [O.harmonic_embedding(x), O.timestep_embedding(t, sd)[:, None, :].expand(-1, N, -1), z]
    if net.pivot:
        pivot = torch.zeros_like(z[..., :1])
        pivot[:, 0] = 1.0
        parts.append(pivot)
    h = torch.cat(parts, dim=-1) @ sd["_first.weight"].T + sd["_first.bias"]
    d = h.shape[-1]
    dh = d // net.nhead
    out = []
    for l in range(net.layers):
        p = f"_trunk.layers.{l}."
        a = O._layer_norm(h, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
        qkv = a @ sd[p + "self_attn.in_proj_weight"].T + sd[p + "self_attn.in_proj_bias"]
        q, k, v = (u.reshape(B, N, net.nhead, dh).transpose(1, 2) for u in qkv.split(d, dim=-1))
        lg = torch.log_softmax((q / math.sqrt(dh)) @ k.transpose(-1, -2), dim=-1)
        out.append(lg)
        ctx = (lg.exp() @ v).transpose(1, 2).reshape(B, N, d)
        h = h + (ctx @ sd[p + "self_attn.out_proj.weight"].T + sd[p + "self_attn.out_proj.bias"])
        a = O._layer_norm(h, sd[p + "norm2.weight"], sd[p + "norm2.bias"])
        a = torch.relu(a @ sd[p + "linear1.weight"].T + sd[p + "linear1.bias"])
        h = h + (a @ sd[p + "linear2.weight"].T + sd[p + "linear2.bias"])
    return out


def attention_probs(sd: Dict[str, torch.Tensor], net: TC.Net, inp: Dict[str, torch.Tensor]) -> List[torch.Tensor]:
    """The softmax rows [B, nhead, N, N] of every encoder layer in float64."""
    with torch.no_grad():
        sd = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
        x = TC.q_sample(inp["x_start"].double(), inp["noise"].double(), inp["t"], O.diffusion_tables(dtype=torch.float64))
        return [lg.exp() for lg in _log_probs(sd, net, x, inp["t"], inp["z"].double())]


def fit_last_tile(sd: Dict[str, torch.Tensor], net: TC.Net, inp: Dict[str, torch.Tensor], steps: int = 30) -> Dict[str, torch.Tensor]:
    """``inp`` with the features z of the frames of the LAST key tile (frames 128, 129 at N = 130) fitted so that their keys attract row
    maxima.  Under drawn inputs the row maximum of a sharp softmax falls on a key chosen almost uniformly (measured: no key holds more
    than 2.2 % of the rows), so a tile of 2 keys out of 130 holds 1.5 % of them, whatever the seed; ``steps`` Adam steps in float64 on
    the CPU raise the probability mass those two keys receive (capped at 0.7 per row, so the other tiles keep their share).  Only z of
    those frames changes, by the size of z's own entries; the caller asserts the precondition on the result."""
    sd = {k: v.detach().double() for k, v in sd.items() if v.is_floating_point()}
    N = inp["x_start"].shape[1]
    first = (N - 1) // TILE * TILE
    x = TC.q_sample(inp["x_start"].double(), inp["noise"].double(), inp["t"], O.diffusion_tables(dtype=torch.float64))
    head = inp["z"].double()[:, :first]
    tail = inp["z"].double()[:, first:].clone().requires_grad_(True)
    opt = torch.optim.Adam([tail], lr=0.05)
    for _ in range(steps):
        lgs = _log_probs(sd, net, x, inp["t"], torch.cat([head, tail], dim=1))
        mass = sum(torch.logsumexp(lg[..., first:], dim=-1).clamp(max=math.log(0.7)).mean() for lg in lgs)
        opt.zero_grad()
        (-mass).backward()
        opt.step()
    return dict(inp, z=torch.cat([head, tail.detach()], dim=1).float())


def sharp_precondition(probs: List[torch.Tensor]):
    """-> (median over all softmax rows of the largest probability, [share of the rows whose maximum lies in key tile k])."""
    pm = torch.cat([p.max(dim=-1).values.flatten() for p in probs])
    am = torch.cat([p.argmax(dim=-1).flatten() for p in probs]) // TILE
    nt = (probs[0].shape[-1] + TILE - 1) // TILE
    return pm.median().item(), [(am == k).double().mean().item() for k in range(nt)]


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gpu_train_long.py
# 1. tile edges, no dropout: (B, N, objective, loss_type) on "two"
EDGE_CASES = [(1, 65, "pred_noise", "l1"), (2, 128, "pred_noise", "l1"), (1, 129, "pred_noise", "l1"), (1, 192, "pred_noise", "l1"),
              (1, 193, "pred_noise", "l1"), (2, 256, "pred_noise", "l1"), (1, 255, "pred_x0", "l2")]
# 3. dropout, in train_dropout_checks.GPU_CASES' layout: (name, configuration, B, N, p, sites, seed, step, objective, loss_type)
DROPOUT_CASES = (
    [(f"long_site{s}_p{p}", "two", 1, 65, p, s, 31, 0, "pred_noise", "l1") for s in (D.ATTN, D.ALL) for p in (0.1, 0.5)]
    + [("long_b2n256", "two", 2, 256, 0.1, D.ALL, 32, 0, "pred_noise", "l1"),
       ("long_b1n130_step3", "two", 1, 130, 0.1, D.ALL, 33, 3, "pred_noise", "l1")])
# 5. bitwise against the short kernels: all sites at p = 0.5 on "two", B = 3
BITWISE_NS = (1, 5, 63, 64)
BITWISE_DROP = dict(dropout_p=0.5, dropout_sites=D.ALL, seed=41, step=1)
BITWISE_CASES = [(f"bitwise_n{n}", "two", 3, n, 0.5, D.ALL, 41, 1, "pred_noise", "l1") for n in BITWISE_NS]
# 6. determinism and capacity: the batches one (4, 256) trainer runs in turn, all sites at p = 0.1
CAPACITY_BATCHES = [(2, 256), (3, 7), (1, 65), (2, 130), (3, 7)]
CAPACITY_DROP = dict(dropout_p=0.1, dropout_sites=D.ALL, seed=51, step=0)
CAPACITY_CASES = [(f"capacity_b{b}n{n}", "two", b, n, 0.1, D.ALL, 51, 0, "pred_noise", "l1") for b, n in sorted(set(CAPACITY_BATCHES))]
MASKED_CASES = DROPOUT_CASES + BITWISE_CASES + CAPACITY_CASES          # every case whose masks tests/test_train_long_cpu.py checks
# 4. sharp softmax across tiles: "two" with W_q and W_k x 4 at (SHARP_B, 130), inputs fit_last_tile(test_gpu_train_grad._inputs(.., seed = SHARP_SEED))
SHARP_B, SHARP_N, SHARP_QK, SHARP_SEED = 1, 130, 4.0, 0


def make_two(qk_factor: float = 1.0):
    """The Denoiser of train_dropout_checks.CONFIGS["two"] (the default shape with 2 encoder layers, seeded like the dropout suite's);
    ``qk_factor`` multiplies W_q and W_k, so every score is qk_factor^2 larger."""
    from posediffusion_amd import synth
    two = synth.make_diffuser(seed=0, num_layers=2)
    synth.randomize_norm_and_bias_(two.model)
    if qk_factor != 1.0:
        with torch.no_grad():
            for layer in two.model._trunk.layers:
                d = layer.self_attn.in_proj_weight.shape[1]
                layer.self_attn.in_proj_weight[:2 * d] *= qk_factor
    return two.model


def check_sharp_precondition(sd, net: TC.Net, inp) -> None:
    """On float64 alone: the median largest probability is >= 0.5 and each key tile holds the row maximum of >= 10 % of the query rows."""
    med, shares = sharp_precondition(attention_probs(sd, net, inp))
    print(f"sharp N = {inp['x_start'].shape[1]}: median largest probability {med:.3f}; share of the row maxima per key tile {[f'{s:.3f}' for s in shares]}")
    assert med >= 0.5, med
    assert len(shares) == 3 and all(s >= 0.10 for s in shares), shares
