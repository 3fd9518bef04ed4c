"""VitTrainer: thin Python owner of a ``pd_vit_trainer`` (include/pd_engine_vit_train.h) -- the averaged multi-scale CLS features of
MultiScaleImageFeatureExtractor (models/image_feature_extractor.py:57-87) around the DINO ViT-S/16 and, given dS/dz, the gradient of
every backbone parameter, computed by hand-written gfx950 kernels from the LIVE PyTorch parameters: an optimiser step needs no rebuild,
no LayerNorm folding and no repacking (``VitEngine``, the inference path, keeps repacked copies and is untouched).

``multiscale_with_grad`` is the ``torch.autograd.Function`` that hands the engine's gradients to autograd; PyTorch keeps the optimiser.
DINO's ``interpolate_pos_encoding`` (bicubic resampling of the trained position grid) is evaluated with torch at every call from the
live ``pos_embed`` -- nothing is cached, so nothing can go stale; its adjoint runs on the engine.  (One geometry is written out instead:
the trained grid under unequal pixel sizes, where torch's GPU kernel copies -- ``_pos_for``.)  Exact fp32, at most 256 tokens per
image and scale (240 x 272 pixels).  Images are data: no image gradient.  No CPU path: a missing library or GPU raises."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, List, Optional, Sequence

import torch
import torch.nn.functional as F

from . import _lib

PATCH = 16
MAX_TOKENS = _lib.PD_VIT_TRAIN_MAX_TOKENS
_TOP = (("patch_embed.proj.weight", "patch_w"), ("patch_embed.proj.bias", "patch_b"), ("cls_token", "cls_token"), ("pos_embed", "pos_embed"),
        ("norm.weight", "norm_w"), ("norm.bias", "norm_b"))
_LAYER = (("norm1.weight", "norm1_w"), ("norm1.bias", "norm1_b"), ("attn.qkv.weight", "qkv_w"), ("attn.qkv.bias", "qkv_b"),
          ("attn.proj.weight", "proj_w"), ("attn.proj.bias", "proj_b"), ("norm2.weight", "norm2_w"), ("norm2.bias", "norm2_b"),
          ("mlp.fc1.weight", "fc1_w"), ("mlp.fc1.bias", "fc1_b"), ("mlp.fc2.weight", "fc2_w"), ("mlp.fc2.bias", "fc2_b"))


def param_names(depth: int) -> List[str]:
    """The DINO ViT's parameters under their state-dict names, in pd_vit_weights' order."""
    names = [n for n, _ in _TOP]
    for l in range(depth):
        names += [f"blocks.{l}.{n}" for n, _ in _LAYER]
    return names


def shape_from_module(net: torch.nn.Module) -> Dict:
    """The shape fields of pd_vit_weights, read off a live DINO parameter tree (the drop-in's ``_net`` or the oracle's ``DinoViT``)."""
    n_pos = net.pos_embed.shape[-2]
    return {"dim": int(net.pos_embed.shape[-1]), "depth": len(net.blocks), "num_heads": 6, "mlp_hidden": int(net.blocks[0].mlp.fc1.weight.shape[0]),
            "patch_size": int(net.patch_embed.proj.weight.shape[-1]), "pos_grid": int(round(math.sqrt(n_pos - 1)))}


def scaled_size(H: int, W: int, sf: float):
    """Pixels of one scale: F.interpolate's floor(size * scale_factor) in double; a scale of 1 keeps the image."""
    return (H, W) if sf == 1 else (int(math.floor(H * float(sf))), int(math.floor(W * float(sf))))


def token_rows(H: int, W: int, scale_factors: Sequence[float]) -> int:
    """Token rows one image takes over the scales of a call (the unit of ``VitTrainer``'s capacity)."""
    return sum(1 + (hs // PATCH) * (ws // PATCH) for hs, ws in (scaled_size(H, W, sf) for sf in scale_factors))


def _bicubic_matrix(g_out: int, g: int) -> torch.Tensor:
    """[g_out, g] float32 on the CPU: one axis of torch's bicubic upsample (A = -0.75, align_corners=False) of a g-long grid onto g_out cells
    under DINO's scale factor (g_out + 0.1) / g -- source coordinate float(1 / scale_factor) (o + 0.5) - 0.5, not clamped, the four taps
    clamped to [0, g - 1] (pd_vt_cubic_taps' arithmetic)."""
    rscale = torch.tensor(1.0 / ((g_out + 0.1) / g), dtype=torch.float32)
    src = rscale * (torch.arange(g_out, dtype=torch.float32) + 0.5) - 0.5
    fl = torch.floor(src)
    t = src - fl

    def near(x):                    # |x| <= 1
        return ((1.25 * x - 2.25) * x) * x + 1.0

    def far(x):                     # 1 < |x| < 2
        return ((-0.75 * x + 3.75) * x - 6.0) * x + 3.0
    m = torch.zeros(g_out, g)
    for k, w in enumerate((far(t + 1.0), near(t), near(1.0 - t), far(2.0 - t))):
        m.index_put_((torch.arange(g_out), (fl.long() - 1 + k).clamp(0, g - 1)), w, accumulate=True)
    return m


def _fill(struct, depth: int, ptr_of) -> None:
    """struct.<field> = ptr_of(state-dict name) for every pointer member of pd_vit_weights / pd_vit_weight_grads"""
    for name, field in _TOP:
        setattr(struct, field, ptr_of(name))
    for l in range(depth):
        for name, field in _LAYER:
            setattr(struct.layers[l], field, ptr_of(f"blocks.{l}.{name}"))


class VitTrainer:
    """``shape``: ``shape_from_module(net)``.  Capacity: ``max_images`` images per call and ``max_rows`` token rows summed over the scales
    of one call (``n * token_rows(H, W, scale_factors)``), ``max_scales`` scales."""

    def __init__(self, shape: Dict, max_images: int, max_rows: int, max_scales: int = 3, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("posediffusion_amd.VitTrainer needs an AMD GPU (torch.cuda unavailable); there is no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else "cuda:0")
        self.shape = dict(shape)
        self.depth = int(shape["depth"])
        self.dim, self.grid0 = int(shape["dim"]), int(shape["pos_grid"])
        self.max_images, self.max_rows, self.max_scales = int(max_images), int(max_rows), int(max_scales)
        self.names = param_names(self.depth)
        self._h = C.c_void_p(None)
        self._generation = 0                 # bumped by every forward: a backward belongs to the LAST forward only
        self._pending = None                 # n of the forward whose stash is waiting for its backward
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            _lib.check(self.lib.pd_vit_trainer_create(C.byref(self._weights_struct(None)), self.max_images, self.max_rows, self.max_scales,
                                                      C.byref(self._h)), "pd_vit_trainer_create")

    def _weights_struct(self, params: Optional[Dict[str, torch.Tensor]]) -> _lib.pd_vit_weights:
        s = self.shape
        w = _lib.pd_vit_weights()
        w.dim, w.depth, w.num_heads, w.mlp_hidden = int(s["dim"]), int(s["depth"]), int(s["num_heads"]), int(s["mlp_hidden"])
        w.patch_size, w.pos_grid = int(s["patch_size"]), int(s["pos_grid"])
        if params is not None:
            _fill(w, min(self.depth, len(w.layers)), lambda n: params[n].data_ptr())
        return w

    def _live(self, params: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The caller's tensors themselves (fp32, contiguous, on the device): nothing is copied, so a non-conforming one is an error."""
        out = {}
        for n in self.names:
            t = params[n].detach()
            if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"parameter {n} must be a contiguous float32 tensor on {self.device} (got {t.dtype} on {t.device}): "
                                 "the trainer reads the live tensors and keeps no copy")
            out[n] = t
        return out

    # ---------------------------------------------------------------- lifecycle
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.pd_vit_trainer_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _pos_for(self, pos_embed: torch.Tensor, hs: int, ws: int) -> Optional[torch.Tensor]:
        """DINO interpolate_pos_encoding of the LIVE table for an hs x ws pixel input -> [1 + gh gw, dim], or None for the trained grid
        (``VitEngine._pos_for``'s rule, evaluated per call)."""
        gh, gw, g = hs // PATCH, ws // PATCH, self.grid0
        if (gh == g and gw == g and hs == ws) or gh < 1 or gw < 1:       # (no whole patch: pd_vit_train_forward refuses the scale and names the limit)
            return None
        pe = pos_embed.detach().reshape(1, 1 + g * g, self.dim)
        if gh == g and gw == g:
            # The trained grid under unequal pixel sizes (224 x 232).  DINO resamples it with scale factor (g + 0.1) / g per axis, and the
            # reference's float64 CPU kernel evaluates that: source coordinates move by up to 0.1 cell.  torch's GPU bicubic kernel COPIES
            # whenever input and output sizes are equal, whatever the scale factor, so here the resampling is written out as its two tap
            # matrices (the taps pd_vt_posgrid_kernel's adjoint uses).
            m = _bicubic_matrix(g, g).to(pe.device)
            pp = torch.einsum("yi,xj,ijc->yxc", m, m, pe[0, 1:].reshape(g, g, self.dim))
            return torch.cat((pe[0, :1], pp.reshape(-1, self.dim)), dim=0).contiguous()
        # (DINO names the first spatial size w; it passes (w0 / g, h0 / g) for the (rows, cols) of the grid)
        w0, h0 = gh + 0.1, gw + 0.1
        pp = F.interpolate(pe[:, 1:].reshape(1, g, g, self.dim).permute(0, 3, 1, 2), scale_factor=(w0 / g, h0 / g), mode="bicubic")
        if (int(w0), int(h0)) != tuple(pp.shape[-2:]):
            raise RuntimeError("position-grid resampling produced an unexpected size")
        return torch.cat((pe[0, :1], pp.permute(0, 2, 3, 1).reshape(-1, self.dim)), dim=0).contiguous()

    # ---------------------------------------------------------------- forward / backward
    def forward(self, params: Dict[str, torch.Tensor], images: torch.Tensor, scale_factors: Sequence[float] = (1, 1 / 2, 1 / 3)) -> torch.Tensor:
        """pd_vit_train_forward: images [n, 3, H, W] in [0, 1] -> z [n, dim] from the live ``params`` (DINO state-dict names -> tensors),
        with the stash one ``backward`` consumes.  A refused call (too many tokens, beyond capacity) raises and leaves the trainer usable."""
        if len(scale_factors) <= 0:
            raise ValueError(f"Wrong format of self.scale_factors: {scale_factors}")                    # image_feature_extractor.py:68-69
        live = self._live(params)
        x = images.detach().to(device=self.device, dtype=torch.float32).contiguous()
        n, _, H, W = x.shape
        with torch.no_grad():
            tables = [self._pos_for(live["pos_embed"], *scaled_size(H, W, sf)) for sf in scale_factors]
        sfs = (C.c_double * len(scale_factors))(*[float(sf) for sf in scale_factors])
        pos = (C.c_void_p * len(scale_factors))(*[None if t is None else t.data_ptr() for t in tables])
        z = torch.empty(n, self.dim, device=self.device)
        w = self._weights_struct(live)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.pd_vit_train_forward(self._h, C.byref(w), x.data_ptr(), n, H, W, sfs, len(scale_factors), pos, z.data_ptr(),
                                                     self._stream()), "pd_vit_train_forward")
        self._generation += 1                # (a refused call raised above: generation and pending stash are as they were)
        self._pending = n
        return z

    def backward(self, params: Dict[str, torch.Tensor], g_z: torch.Tensor, want: Optional[Iterable[str]] = None) -> Dict[str, torch.Tensor]:
        """pd_vit_train_backward: ``{name: dS/d param}`` for g_z = dS/dz [n, dim] and the names in ``want`` (state-dict names; default:
        every parameter).  ``params`` must be the tensors of the forward, unmodified.  A name left out is not computed."""
        if self._pending is None:                # pd_vit_train_backward itself refuses (PD_ERR_STATE): its message is the one raised
            dummy = torch.zeros(1, device=self.device)
            _lib.check(self.lib.pd_vit_train_backward(self._h, C.byref(self._weights_struct(None)), dummy.data_ptr(),
                                                      C.byref(_lib.pd_vit_weight_grads()), self._stream()), "pd_vit_train_backward")
            raise RuntimeError("pd_vit_train_backward accepted a call without a pending forward")
        n = self._pending
        want = set(self.names) if want is None else set(want)
        unknown = want - set(self.names)
        if unknown:
            raise KeyError(f"unknown gradient names {sorted(unknown)}")
        live = self._live(params)
        g_z = g_z.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(g_z.shape) != (n, self.dim):
            raise ValueError(f"expected g_z of shape {(n, self.dim)}, got {tuple(g_z.shape)}")
        grads = {k: torch.empty_like(live[k]) for k in self.names if k in want}
        g = _lib.pd_vit_weight_grads()
        _fill(g, self.depth, lambda k: grads[k].data_ptr() if k in grads else None)
        w = self._weights_struct(live)
        self._pending = None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.pd_vit_train_backward(self._h, C.byref(w), g_z.data_ptr(), C.byref(g), self._stream()), "pd_vit_train_backward")
        return grads


class _MultiScaleFn(torch.autograd.Function):
    """(trainer, scale_factors, images, *params) -> z, differentiable with respect to the parameters (passed flat so that autograd routes
    their gradients); images get no gradient."""

    @staticmethod
    def forward(ctx, trainer, scale_factors, images, *params):
        z = trainer.forward(dict(zip(trainer.names, params)), images, scale_factors)
        ctx.trainer, ctx.generation = trainer, trainer._generation
        ctx.save_for_backward(*params)
        return z

    @staticmethod
    def backward(ctx, g_z):
        tr = ctx.trainer
        if ctx.generation != tr._generation or tr._pending is None:
            raise RuntimeError("VitTrainer keeps ONE activation stash: backward must follow its own forward, once, before the next forward "
                               "on the same trainer (no retain_graph, no two feature batches in flight)")
        params = ctx.saved_tensors
        want = [n for n, need in zip(tr.names, ctx.needs_input_grad[3:]) if need]
        grads = tr.backward(dict(zip(tr.names, params)), g_z, want)
        return (None, None, None) + tuple(grads.get(n) for n in tr.names)


def multiscale_with_grad(trainer: VitTrainer, net: torch.nn.Module, images: torch.Tensor, scale_factors: Sequence[float] = (1, 1 / 2, 1 / 3)) -> torch.Tensor:
    """``trainer.forward``'s z attached to ``net``'s parameters (a DINO parameter tree: the drop-in's ``_net``)."""
    named = dict(net.named_parameters())
    return _MultiScaleFn.apply(trainer, tuple(scale_factors), images, *[named[n] for n in trainer.names])
