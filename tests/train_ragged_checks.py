"""Yardstick of the trainer's frame counts (pd_trainer_set_frame_counts, include/pd_engine_train.h): train_checks' teacher-forced
float64 / float32 p_losses -- with train_dropout_checks' four dropout sites when asked for -- on the PADDED layout [B, N, .] in which
sequence b has n_frames[b] frames in rows 0 .. n_frames[b]-1 of its N-row block.  Written from the contract in the header, not from
the kernels:

  * inputs (x_start, noise, z) are zeroed at padding rows (a select, so that what they hold -- NaN included -- is not read);
  * attention scores of keys >= n_frames[b] are -inf before the softmax; every query row, padding rows included, keeps its keys
    < n_frames[b] (a count is at least 1), so no softmax row is empty;
  * dropout masks come from ``keep_mask`` on the PADDED shapes: rows (b nhead + h) N + i and m = b N + i with the padded N;
  * g_loss is zero at padding; ``None`` means 1 / (9 sum(n_frames)) on the valid rows -- the mean loss over real frames;
  * ReLU masks and l1 signs are forced as in ``train_checks.loss_and_grads``.
Padding rows of loss, model_out and x_t are returned as +0, and dz is exactly zero there (the select's gradient).  With all counts = N
every operation is the one ``loss_and_grads`` / ``loss_and_grads_dropout`` performs (a select that takes every element, a fill that
fills none), so the result is theirs bit for bit; tests/test_train_ragged_checks_cpu.py pins that, the agreement with the sum over the
sequences run alone, and the independence of the padding rows' contents.
Shared by tests/test_train_ragged_checks_cpu.py, tests/test_gpu_train_ragged.py and tests/test_gpu_train_ragged_exact.py."""
from __future__ import annotations

import math
from typing import Dict, Sequence

import torch

from oracle import pd_oracle as O
import train_checks as TC
import train_dropout_checks as TD


def valid_rows(n_frames: Sequence[int], N: int) -> torch.Tensor:
    """[B, N] bool: True where row i of sequence b is a frame (i < n_frames[b])."""
    nf = torch.as_tensor(list(n_frames), dtype=torch.long)
    assert nf.dim() == 1 and int(nf.min()) >= 1 and int(nf.max()) <= N, (list(n_frames), N)
    return torch.arange(N)[None, :] < nf[:, None]


def zero_padding(x: torch.Tensor, valid: torch.Tensor) -> torch.Tensor:
    """x [B, N, .] with +0 at padding rows, by a select."""
    return torch.where(valid[..., None], x, torch.zeros((), dtype=x.dtype))


def attention(sd: Dict[str, torch.Tensor], prefix: str, a: torch.Tensor, nhead: int, layer: int, sites: int, drop, valid, pmax=None):
    """train_dropout_checks.attention with the scores of padding keys at -inf."""
    B, N, d = a.shape
    dh = d // nhead
    qkv = a @ sd[prefix + "self_attn.in_proj_weight"].T + sd[prefix + "self_attn.in_proj_bias"]
    q, k, v = (u.reshape(B, N, nhead, dh).transpose(1, 2) for u in qkv.split(d, dim=-1))
    scores = ((q / math.sqrt(dh)) @ k.transpose(-1, -2)).masked_fill(~valid[:, None, None, :], float("-inf"))
    att = torch.softmax(scores, dim=-1)
    if pmax is not None:
        pmax.append(att.detach().max(dim=-1).values)
    if sites & TD.ATTN:
        att = att * TD._keep(B * nhead * N, N, layer, 0, drop, a.dtype).reshape(B, nhead, N, N)
    ctx = (att @ v).transpose(1, 2).reshape(B, N, d)
    return ctx @ sd[prefix + "self_attn.out_proj.weight"].T + sd[prefix + "self_attn.out_proj.bias"]


def encoder_layer(sd, prefix: str, h, nhead: int, layer: int, sites: int, drop, valid, relu_mask, pre, used, pmax):
    """train_dropout_checks.encoder_layer around the attention above."""
    B, N, d = h.shape
    o = attention(sd, prefix, O._layer_norm(h, sd[prefix + "norm1.weight"], sd[prefix + "norm1.bias"]), nhead, layer, sites, drop, valid, pmax)
    if sites & TD.RESID1:
        o = o * TD._keep(B * N, d, layer, 1, drop, h.dtype).reshape(B, N, d)
    h = h + o
    a = O._layer_norm(h, sd[prefix + "norm2.weight"], sd[prefix + "norm2.bias"])
    a = TC._relu(a @ sd[prefix + "linear1.weight"].T + sd[prefix + "linear1.bias"], relu_mask, pre, used)
    if sites & TD.FF:
        a = a * TD._keep(B * N, a.shape[-1], layer, 2, drop, h.dtype).reshape(a.shape)
    o = a @ sd[prefix + "linear2.weight"].T + sd[prefix + "linear2.bias"]
    if sites & TD.RESID2:
        o = o * TD._keep(B * N, d, layer, 3, drop, h.dtype).reshape(B, N, d)
    return h + o


def denoiser_forward(sd, net: TC.Net, x, t, z, valid, sites: int = 0, drop=(0.0, 0, 0), masks=None):
    """train_checks.denoiser_forward on the padded layout; same return value (info["pmax"]: [B, nhead, N] per layer, over valid keys)."""
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
        h = encoder_layer(sd, f"_trunk.layers.{l}.", h, net.nhead, l, sites, drop, valid, None if masks is None else masks[l], pre, used, pmax)
    a = O._layer_norm(h @ sd["_last.0.weight"].T + sd["_last.0.bias"], sd["_last.1.weight"], sd["_last.1.bias"])
    a = TC._relu(a, None if masks is None else masks[net.layers], pre, used)
    return a @ sd["_last.3.weight"].T + sd["_last.3.bias"], {"pre": pre, "masks": used, "pmax": pmax}


def default_g_loss(n_frames: Sequence[int], N: int, dtype=torch.float64) -> torch.Tensor:
    """[B, N, 9]: 1 / (9 sum(n_frames)) on valid rows, 0 at padding -- S is then the mean loss over real frames."""
    valid = valid_rows(n_frames, N)
    g = torch.full((len(n_frames), N, 9), 1.0 / (9 * int(sum(int(v) for v in n_frames))), dtype=dtype)
    return zero_padding(g, valid)


def loss_and_grads(sd, net: TC.Net, inp, n_frames: Sequence[int], objective: str, loss_type: str, g_loss=None, masks=None, signs=None,
                   dtype=torch.float64, want=None, p: float = 0.0, sites: int = 0, seed: int = 0, step: int = 0):
    """train_checks.loss_and_grads / train_dropout_checks.loss_and_grads_dropout with frame counts: same arguments, same result dict
    (plus "valid" [B, N] and "pmax").  Gradients are those of S = sum(g_loss * loss) over the valid rows."""
    if p == 0.0:
        sites = 0
    sd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    tables = O.diffusion_tables(dtype=dtype)
    B, N, _ = inp["x_start"].shape
    valid = valid_rows(n_frames, N)
    assert valid.shape[0] == B
    x_start, noise, t = zero_padding(inp["x_start"].to(dtype), valid), zero_padding(inp["noise"].to(dtype), valid), inp["t"]
    z_leaf = inp["z"].detach().to(dtype).requires_grad_(True)
    z = zero_padding(z_leaf, valid)
    x_t = TC.q_sample(x_start, noise, t, tables)
    out, info = denoiser_forward(sd, net, x_t, t, z, valid, sites, (p, seed, step), masks)
    target = noise if objective == "pred_noise" else x_start
    d = out - target
    if loss_type == "l1":
        s = torch.sign(d.detach()) if signs is None else signs.to(dtype).reshape(d.shape)
        loss = d * s
    else:
        s = torch.sign(d.detach())
        loss = d * d
    g = torch.full_like(loss, 1.0 / (9 * int(valid.sum()))) if g_loss is None else g_loss.to(dtype).reshape(loss.shape)
    g = zero_padding(g, valid)
    names = list(sd) if want is None else [n for n in want if n != "z"]
    gs = torch.autograd.grad((g * loss).sum(), [sd[n] for n in names] + [z_leaf], allow_unused=True)
    grads = {n: (torch.zeros_like(sd[n]) if v is None else v) for n, v in zip(names, gs[:-1])}
    grads["z"] = gs[-1]
    return {"loss": zero_padding(loss.detach(), valid), "model_out": zero_padding(out.detach(), valid), "x_t": x_t.detach(),
            "target": target, "grads": grads, "pre": info["pre"], "masks": info["masks"], "signs": s, "valid": valid, "pmax": info["pmax"]}


def slice_sequence(inp: Dict[str, torch.Tensor], b: int, n: int) -> Dict[str, torch.Tensor]:
    """Sequence b alone with its n frames: the inputs of a (1, n) call."""
    return {"x_start": inp["x_start"][b:b + 1, :n], "noise": inp["noise"][b:b + 1, :n], "z": inp["z"][b:b + 1, :n], "t": inp["t"][b:b + 1]}
