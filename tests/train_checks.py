"""Teacher-forced gradient yardstick for the training branch (include/pd_engine_train.h): a differentiable float64 / float32 restatement
of the pre-norm Denoiser forward (models/denoiser.py:53-76; pivot on or off) and of the p_losses loss (gaussian_diffuser.py:308-327) in
which every ReLU is ``a * mask`` and |d| is ``d * s`` with ``mask`` and ``s`` given as CONSTANTS.

Why: the gradient is discontinuous at every ReLU threshold and at d = 0 under l1 -- one activation that lands on the other side of zero
in fp32 than in fp64 changes a whole weight-gradient row (the reference's own fp32 autograd is 3e-2 from fp64 at 800 token rows through
5 flipped activations of 6.6 million).  With the masks forced the function is smooth and a 4 x "own fp32 distance" bound is meaningful.
Gradients come from torch.autograd.grad.  Shared by tests/test_train_checks_cpu.py, tests/test_gpu_train_grad.py,
tests/test_gpu_train_grad_edges.py and tools/make_p_losses_grad_golden.py."""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional

import torch

from oracle import pd_oracle as O


class Net(NamedTuple):
    layers: int
    nhead: int
    pivot: bool

    @staticmethod
    def of_cfg(cfg) -> "Net":                     # a denoiser_cfgs.Cfg
        assert cfg.norm_first, "the trainer (and this helper) is pre-norm only"
        return Net(cfg.layers, cfg.heads, cfg.pivot)


DEFAULT_NET = Net(8, 4, True)


def _relu(a: torch.Tensor, mask: Optional[torch.Tensor], pre: List[torch.Tensor], used: List[torch.Tensor]) -> torch.Tensor:
    pre.append(a.detach())
    m = (a.detach() > 0) if mask is None else mask.reshape(a.shape)
    used.append(m)
    return a * m.to(a.dtype)


def denoiser_forward(sd: Dict[str, torch.Tensor], net: Net, x: torch.Tensor, t: torch.Tensor, z: torch.Tensor, masks=None):
    """-> (model_out [B, N, 9], info) with info["pre"] = the L + 1 ReLU inputs ([B, N, ff] per layer, then _last's [B, N, hidden]) and
    info["masks"] = the boolean masks used (``masks`` when given, else ``pre > 0``); info["pmax"] = per layer the largest probability
    of every softmax row ([B, nhead, N]), how far from uniform (1 / N) the attention is."""
    B, N, _ = x.shape
    pre, used, pmax = [], [], []
    t_emb = O.timestep_embedding(t, sd)[:, None, :].expand(-1, N, -1)
    parts = [O.harmonic_embedding(x), t_emb, z]
    if net.pivot:
        pivot = torch.zeros_like(z[..., :1])
        pivot[:, 0] = 1.0
        parts.append(pivot)
    h = torch.cat(parts, dim=-1) @ sd["_first.weight"].T + sd["_first.bias"]
    d = h.shape[-1]
    dh = d // net.nhead
    for l in range(net.layers):
        p = f"_trunk.layers.{l}."
        a = O._layer_norm(h, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
        qkv = a @ sd[p + "self_attn.in_proj_weight"].T + sd[p + "self_attn.in_proj_bias"]
        q, k, v = (u.reshape(B, N, net.nhead, dh).transpose(1, 2) for u in qkv.split(d, dim=-1))
        att = torch.softmax((q / math.sqrt(dh)) @ k.transpose(-1, -2), dim=-1)
        pmax.append(att.detach().max(dim=-1).values)
        ctx = (att @ v).transpose(1, 2).reshape(B, N, d)
        h = h + (ctx @ sd[p + "self_attn.out_proj.weight"].T + sd[p + "self_attn.out_proj.bias"])
        a = O._layer_norm(h, sd[p + "norm2.weight"], sd[p + "norm2.bias"])
        a = _relu(a @ sd[p + "linear1.weight"].T + sd[p + "linear1.bias"], None if masks is None else masks[l], pre, used)
        h = h + (a @ sd[p + "linear2.weight"].T + sd[p + "linear2.bias"])
    a = O._layer_norm(h @ sd["_last.0.weight"].T + sd["_last.0.bias"], sd["_last.1.weight"], sd["_last.1.bias"])
    a = _relu(a, None if masks is None else masks[net.layers], pre, used)
    return a @ sd["_last.3.weight"].T + sd["_last.3.bias"], {"pre": pre, "masks": used, "pmax": pmax}


def q_sample(x_start, noise, t, tables):
    at = lambda name: tables[name][t].reshape(-1, 1, 1)                         # noqa: E731
    return at("sqrt_alphas_cumprod") * x_start + at("sqrt_one_minus_alphas_cumprod") * noise


def loss_and_grads(sd: Dict[str, torch.Tensor], net: Net, inp: Dict[str, torch.Tensor], objective: str, loss_type: str, g_loss=None,
                   masks=None, signs=None, dtype=torch.float64, want=None):
    """p_losses in ``dtype`` with forced ``masks`` / ``signs`` (None: the function's own) and the gradients of S = sum(g_loss * loss)
    (g_loss None: 1 / numel, i.e. loss.mean()) with respect to every entry of ``sd`` (or the names in ``want``) and "z".
    -> dict(loss, model_out, x_t, target, grads {name: tensor}, pre, masks, signs)."""
    sd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    tables = O.diffusion_tables(dtype=dtype)
    x_start, noise, t = inp["x_start"].to(dtype), inp["noise"].to(dtype), inp["t"]
    z = inp["z"].detach().to(dtype).requires_grad_(True)
    x_t = q_sample(x_start, noise, t, tables)
    out, info = denoiser_forward(sd, net, x_t, t, z, masks)
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


def draw_g_loss(B: int, N: int, seed: int = 0) -> torch.Tensor:
    """A non-uniform upstream gradient [B, N, 9] (a masked, per-frame-weighted loss): randn / (B N 9), so mixed signs, times a per-frame
    factor that spans three decades over the B N frames; sequence 0 entirely and frame 1 of every sequence are zero."""
    g = torch.Generator().manual_seed(7700 + 100 * B + N + seed)
    w = (10.0 ** torch.linspace(-3.0, 0.0, B * N))[torch.randperm(B * N, generator=g)].reshape(B, N, 1)
    out = torch.randn(B, N, 9, generator=g) / (B * N * 9) * w
    out[0] = 0.0
    out[:, 1] = 0.0
    return out


def grad_dist(g, g64) -> float:
    """max|g - g64| / max|g64| of one tensor (0 when both are identically zero)."""
    g, g64 = torch.as_tensor(g).detach().cpu().double(), torch.as_tensor(g64).detach().cpu().double()
    den = g64.abs().max().item()
    num = (g - g64).abs().max().item()
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den


FIRST_FIXED_COLS = (("harmonic", 0, 180), ("x", 180, 189), ("t_emb", 189, 317))       # _first's columns before z (models/denoiser.py:56-68)


def grad_blocks(name: str, g: torch.Tensor, d_model: int, z_dim: int) -> Dict[str, torch.Tensor]:
    """The sub-blocks of the gradient ``g`` of parameter ``name`` that come from different parts of the backward and differ in
    magnitude, so that a whole-tensor maximum norm is decided by one of them: the q, k and v row blocks of ``in_proj_weight`` /
    ``in_proj_bias`` (q and k come from the softmax backward, v from P^T dO and usually dominates), and the column blocks of
    ``_first.weight`` (harmonic, x, t_emb, z and, when the tensor has it, the pivot column).  {} for every other tensor."""
    if name.endswith(("self_attn.in_proj_weight", "self_attn.in_proj_bias")):
        assert g.shape[0] == 3 * d_model, (name, tuple(g.shape))
        return {"q": g[:d_model], "k": g[d_model:2 * d_model], "v": g[2 * d_model:]}
    if name == "_first.weight":
        z0 = FIRST_FIXED_COLS[-1][2]
        assert g.shape[1] in (z0 + z_dim, z0 + z_dim + 1), (name, tuple(g.shape))
        out = {b: g[:, lo:hi] for b, lo, hi in FIRST_FIXED_COLS}
        out["z"] = g[:, z0:z0 + z_dim]
        if g.shape[1] > z0 + z_dim:
            out["pivot"] = g[:, z0 + z_dim:]
        return out
    return {}


def block_dists(name: str, g, g_own, g64, d_model: int, z_dim: int):
    """[(block, distance of g, distance of g_own, zero)] per block of `grad_blocks`, each distance against that block's OWN float64
    maximum (`grad_dist`); ``zero`` = the float64 block is identically zero."""
    b, bo, b64 = (grad_blocks(name, torch.as_tensor(t).detach().cpu(), d_model, z_dim) for t in (g, g_own, g64))
    return [(k, grad_dist(b[k], b64[k]), grad_dist(bo[k], b64[k]), b64[k].abs().max().item() == 0.0) for k in b64]


def block_misses(name: str, g, g_own, g64, d_model: int, z_dim: int, margin: float = 4.0, margins=None):
    """The blocks of `block_dists` whose distance exceeds ``margin`` x own (``margins``: {"name[block]": recorded margin}), or that are
    not exactly zero where float64's is.  The k block of ``in_proj_bias`` is left out: a key bias shifts every score of a softmax row
    equally, so its gradient is mathematically zero and float64 holds only its own rounding there (1e-17 of the tensor's maximum)."""
    out = []
    for k, e, own, zero in block_dists(name, g, g_own, g64, d_model, z_dim):
        if k == "k" and name.endswith("in_proj_bias"):
            continue
        m = (margins or {}).get(f"{name}[{k}]", margin)
        if (zero and e != 0.0) or (not zero and e > m * own):
            out.append((f"{name}[{k}]", e, own))
    return out


# ------------------------------------------------------------------------------------------------ tests/golden/p_losses_grad.npz
GOLDEN_CASE = 1                                  # case b3n5 of p_losses_cases.CASES
GOLDEN_VARIANTS = (("pred_noise", "l1"), ("pred_x0", "l2"))
GOLDEN_SAMPLES = 64
GOLDEN_SEED = 7300


def sample_indices(name_index: int, numel: int) -> torch.Tensor:
    """The GOLDEN_SAMPLES flat indices at which the fixture stores the gradient of parameter tensor number ``name_index``."""
    return torch.randint(0, numel, (GOLDEN_SAMPLES,), generator=torch.Generator().manual_seed(GOLDEN_SEED + name_index))


def make_grad_golden(out_path: str):
    """tests/golden/p_losses_grad.npz from the UNMODIFIED reference's GaussianDiffusion + Denoiser in .eval(), run on CPU through
    oracle/ref_stubs.py (build container only; tools/make_p_losses_grad_golden.py is the command): ``loss.mean().backward()`` of
    p_losses on case b3n5, pred_noise / l1 and pred_x0 / l2.  Per parameter tensor: max|g|, sum(g) and GOLDEN_SAMPLES entries at seeded
    indices -- not the 100 MB of gradients.  Weights are the conftest's seeded ones, stored as a checksum."""
    import os

    import numpy as np

    from oracle import ref_stubs as RS
    from oracle.make_golden import weight_checksum
    from p_losses_cases import CASES, inputs
    from posediffusion_amd import synth
    torch.set_num_threads(1)                      # bit-reproducible reference runs
    diff = RS.build_reference_diffuser(seed=0)
    synth.randomize_norm_and_bias_(diff.model)
    diff.eval()
    inp = inputs(GOLDEN_CASE)
    out = {"weight_checksum": weight_checksum(diff.model.state_dict()), "case": np.array(GOLDEN_CASE), "seed": np.array(GOLDEN_SEED)}
    names = [n for n, _ in diff.model.named_parameters()]
    for obj, lt in GOLDEN_VARIANTS:
        diff.objective, diff.loss_type = obj, lt
        diff.model.zero_grad(set_to_none=True)
        r = diff.p_losses(inp["x_start"], inp["t"], z=inp["z"], noise=inp["noise"])
        r["loss"].mean().backward()
        out[f"{obj}_{lt}_loss_mean"] = np.array(float(r["loss"].detach().mean()))
        gmax, gsum, vals = [], [], []
        for i, (n, p) in enumerate(diff.model.named_parameters()):
            g = p.grad.detach()
            gmax.append(float(g.abs().max()))
            gsum.append(float(g.double().sum()))
            vals.append(g.reshape(-1)[sample_indices(i, g.numel())].numpy())
        out[f"{obj}_{lt}_max"], out[f"{obj}_{lt}_sum"] = np.array(gmax), np.array(gsum)
        out[f"{obj}_{lt}_vals"] = np.stack(vals).astype(np.float32)
    out["n_params"] = np.array(len(names))
    np.savez_compressed(out_path, **out)
    print(f"wrote {out_path} ({os.path.getsize(out_path)} bytes, {len(names)} parameter tensors x {len(GOLDEN_VARIANTS)} variants; case {CASES[GOLDEN_CASE].name})")
