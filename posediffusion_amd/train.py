"""PoseTrainer: thin Python owner of a ``pd_trainer`` (include/pd_engine_train.h) -- the diffusion loss of
GaussianDiffusion.p_losses (models/gaussian_diffuser.py:308-327) and its gradient with respect to every Denoiser parameter (and z),
computed by hand-written gfx950 kernels from the LIVE PyTorch parameters: an optimiser step needs no rebuild and no repacking.

PyTorch keeps the optimiser, the LR schedule and gradient clipping (the reference's train.py:73-77, 245-251); ``p_losses_with_grad``
is the ``torch.autograd.Function`` that hands the engine's gradients to autograd.  Exact fp32, pre-norm only, head dim <= 128, N <= 64
frames by default and up to 256 with ``max_frames`` / ``set_max_frames`` (PD_TR_OPT_MAX_FRAMES): above 64 frames the attention runs
key-tiled kernels, which at N <= 64 give the bits of the default ones (``set_long_attn``, for the tests).
Without ``dropout_p`` it is the eval-mode function; with it, the ``.train()``-mode one: dropout at the four sites of every encoder layer
(``DROPOUT_SITES``), masks from Philox4x32-10 keyed by ``(seed, step)`` and recomputed by the backward (pd_train_forward_dropout).
``n_frames=`` / ``set_frame_counts``: a padded batch whose sequences have different frame counts (pd_trainer_set_frame_counts) --
sequence b has n_frames[b] frames in rows 0 .. of its N-row block, padding rows of every output are +0 and what they hold on input is
never read.  ``loss`` is [B, N, 9] with +0 at padding, so ``loss.mean()`` divides by the PADDED size; the mean over the real frames is
``loss.sum() / (9 * sum(n_frames))``.
No CPU path: a missing library or GPU raises."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Dict, Iterable, List, Optional

import torch

from . import _lib

_LOSS_TYPES = {"l1": 1, "l2": 2}
DROPOUT_SITES = {"attn": _lib.PD_DROP_ATTN, "resid1": _lib.PD_DROP_RESID1, "ff": _lib.PD_DROP_FF, "resid2": _lib.PD_DROP_RESID2}
ALL = _lib.PD_DROP_ALL
_TOP = (("time_embed.linear.0.weight", "time_w0"), ("time_embed.linear.0.bias", "time_b0"), ("time_embed.linear.2.weight", "time_w2"),
        ("time_embed.linear.2.bias", "time_b2"), ("_first.weight", "first_w"), ("_first.bias", "first_b"))
_LAYER = (("norm1.weight", "norm1_w"), ("norm1.bias", "norm1_b"), ("self_attn.in_proj_weight", "in_proj_w"),
          ("self_attn.in_proj_bias", "in_proj_b"), ("self_attn.out_proj.weight", "out_proj_w"), ("self_attn.out_proj.bias", "out_proj_b"),
          ("norm2.weight", "norm2_w"), ("norm2.bias", "norm2_b"), ("linear1.weight", "linear1_w"), ("linear1.bias", "linear1_b"),
          ("linear2.weight", "linear2_w"), ("linear2.bias", "linear2_b"))
_BOTTOM = (("_last.0.weight", "last0_w"), ("_last.0.bias", "last0_b"), ("_last.1.weight", "last_ln_w"), ("_last.1.bias", "last_ln_b"),
           ("_last.3.weight", "last3_w"), ("_last.3.bias", "last3_b"))
_R_TABLES = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")
_Q_TABLES = ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")
DEFAULT_MAX_FRAMES, MAX_FRAMES = 64, 256     # PD_TR_OPT_MAX_FRAMES: its default and its ceiling (PD_MAX_DENOISER_FRAMES)


def param_names(num_layers: int) -> List[str]:
    """The Denoiser's parameters under their state-dict names, in pd_weights' order."""
    names = [n for n, _ in _TOP]
    for l in range(num_layers):
        names += [f"_trunk.layers.{l}.{n}" for n, _ in _LAYER]
    return names + [n for n, _ in _BOTTOM]


def shape_from_modules(denoiser: torch.nn.Module, diffuser: Optional[torch.nn.Module] = None) -> Dict:
    """The shape fields and flags of pd_weights, read off live drop-in (or reference) modules."""
    layer = denoiser._trunk.layers[0]
    pivot = bool(getattr(denoiser, "pivot_cam_onehot", True))
    t_emb_dim = denoiser.time_embed.linear[0].weight.shape[1]
    return {"d_model": denoiser._first.weight.shape[0], "nhead": layer.self_attn.num_heads, "dim_ff": layer.linear1.weight.shape[0],
            "num_layers": len(denoiser._trunk.layers), "mlp_hidden": denoiser._last[0].weight.shape[0], "t_emb_dim": t_emb_dim,
            "z_dim": denoiser._first.weight.shape[1] - (9 * 21 + t_emb_dim // 2 + int(pivot)),
            "norm_first": bool(layer.norm_first), "pivot": pivot,
            "objective": getattr(diffuser, "objective", "pred_noise") if diffuser is not None else "pred_noise"}


def check_frame_counts(n_frames, B: int, N: int) -> List[int]:
    """``n_frames`` as a list of ints after the rule of pd_trainer_set_frame_counts: one count per sequence, each in [1, N]."""
    if isinstance(n_frames, torch.Tensor):
        n_frames = n_frames.detach().cpu().tolist()
    counts = [int(v) for v in n_frames]
    if len(counts) != B:
        raise ValueError(f"n_frames must hold one frame count per sequence ({B}), got {len(counts)}")
    if min(counts) < 1 or max(counts) > N:
        raise ValueError(f"n_frames: every count must lie in [1, N] (N={N}), got {counts}")
    return counts


def _set(struct, field: str, ptr: Optional[int]):
    setattr(struct, field, ptr)


def _fill(struct, num_layers: int, ptr_of) -> None:
    """struct.<field> = ptr_of(state-dict name) for every weight member of pd_weights / pd_weight_grads"""
    for name, field in _TOP + _BOTTOM:
        _set(struct, field, ptr_of(name))
    for l in range(num_layers):
        for name, field in _LAYER:
            _set(struct.layers[l], field, ptr_of(f"_trunk.layers.{l}.{name}"))


class PoseTrainer:
    """``shape``: ``shape_from_modules(...)``; ``tables``: the GaussianDiffusion buffers (the two q_sample tables are required).
    ``max_frames``: frames per sequence ``forward`` admits, 64 (default) .. 256 -- independent of the capacity ``max_N``."""

    def __init__(self, shape: Dict, tables: Dict[str, torch.Tensor], max_B: int, max_N: int, device=None, max_frames: int = DEFAULT_MAX_FRAMES):
        if not torch.cuda.is_available():
            raise RuntimeError("posediffusion_amd.PoseTrainer needs an AMD GPU (torch.cuda unavailable); there is no CPU fallback")
        if shape["objective"] not in ("pred_noise", "pred_x0"):
            raise AssertionError("objective must be either pred_noise (predict noise) or pred_x0 (predict image start)")
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else "cuda:0")
        self.shape = dict(shape)
        self.max_B, self.max_N = int(max_B), int(max_N)
        self.num_layers = int(shape["num_layers"])
        self.names = param_names(self.num_layers)
        self.timesteps = int(tables[_Q_TABLES[0]].shape[0])
        self._h = C.c_void_p(None)
        self._generation = 0                 # bumped by every forward: a backward belongs to the LAST forward only
        self._pending = None                 # (B, N) of the forward whose stash is waiting for its backward
        self._last_shape = None              # (B, N) of the last forward (debug_relu)
        keep = [tables[n].detach().to(device=self.device, dtype=torch.float32).contiguous() for n in _Q_TABLES + _R_TABLES if n in tables]
        ptrs = {n: t.data_ptr() for n, t in zip([n for n in _Q_TABLES + _R_TABLES if n in tables], keep)}
        w = self._weights_struct(None)
        for n in _R_TABLES:
            setattr(w, n, ptrs.get(n))
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            _lib.check(self.lib.pd_trainer_create(C.byref(w), ptrs[_Q_TABLES[0]], ptrs[_Q_TABLES[1]], self.max_B, self.max_N, C.byref(self._h)),
                       "pd_trainer_create")
        del keep
        if int(max_frames) != DEFAULT_MAX_FRAMES:
            try:
                self.set_max_frames(max_frames)
            except Exception:
                self.close()
                raise

    def _weights_struct(self, params: Optional[Dict[str, torch.Tensor]]) -> _lib.pd_weights:
        s = self.shape
        w = _lib.pd_weights()
        w.d_model, w.nhead, w.dim_ff, w.num_layers = int(s["d_model"]), int(s["nhead"]), int(s["dim_ff"]), int(s["num_layers"])
        w.z_dim, w.n_harmonic, w.t_emb_dim, w.mlp_hidden = int(s["z_dim"]), 10, int(s.get("t_emb_dim", 256)), int(s["mlp_hidden"])
        w.timesteps = getattr(self, "timesteps", 0)
        w.reserved = ((_lib.PD_WEIGHTS_PRED_X0 if s["objective"] == "pred_x0" else 0) | (0 if s.get("norm_first", True) else _lib.PD_WEIGHTS_POST_NORM)
                      | (0 if s.get("pivot", True) else _lib.PD_WEIGHTS_NO_PIVOT))
        if params is not None:
            _fill(w, self.num_layers, lambda n: params[n].data_ptr())
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
            self.lib.pd_trainer_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _f32(self, t: torch.Tensor, shape) -> torch.Tensor:
        t = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    # ---------------------------------------------------------------- options
    def set_option(self, option: int, value: int) -> None:
        """pd_trainer_set_option; a refused option or value raises and leaves the old value in force."""
        _lib.check(self.lib.pd_trainer_set_option(self._h, int(option), int(value)), "pd_trainer_set_option")

    def get_option(self, option: int) -> int:
        v = C.c_int(0)
        _lib.check(self.lib.pd_trainer_get_option(self._h, int(option), C.byref(v)), "pd_trainer_get_option")
        return int(v.value)

    def set_max_frames(self, n: int) -> None:
        """Frames per sequence ``forward`` admits from now on: 64 .. 256 (PD_TR_OPT_MAX_FRAMES)."""
        self.set_option(_lib.PD_TR_OPT_MAX_FRAMES, n)

    @property
    def max_frames(self) -> int:
        return self.get_option(_lib.PD_TR_OPT_MAX_FRAMES)

    def set_long_attn(self, on: bool) -> None:
        """True: the key-tiled attention kernels at every N (PD_TR_OPT_LONG_ATTN); at N <= 64 they give the default kernels' bits."""
        self.set_option(_lib.PD_TR_OPT_LONG_ATTN, 1 if on else 0)

    def check_async(self):
        _lib.check(self.lib.pd_trainer_check_async(self._h), "pd_trainer_check_async")

    # ---------------------------------------------------------------- frame counts per sequence
    def set_frame_counts(self, n_frames=None) -> None:
        """pd_trainer_set_frame_counts: ``n_frames`` [B] ints -- sequence b of every later ``forward`` with that B has n_frames[b] frames,
        in rows 0 .. n_frames[b]-1 of its N-row block; the other rows are padding.  ``None`` clears.  A pending stash keeps the counts of
        its own forward.  Ordered on the current stream, no synchronisation; the C entry validates and its message is the one raised."""
        if n_frames is None:
            _lib.check(self.lib.pd_trainer_set_frame_counts(self._h, 0, None, self._stream()), "pd_trainer_set_frame_counts")
            return
        if isinstance(n_frames, torch.Tensor):
            n_frames = n_frames.detach().cpu().tolist()
        counts = [int(v) for v in n_frames]
        arr = (C.c_int32 * max(len(counts), 1))(*counts)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.pd_trainer_set_frame_counts(self._h, len(counts), arr, self._stream()), "pd_trainer_set_frame_counts")

    @contextlib.contextmanager
    def _counts(self, n_frames):
        """The ``n_frames=`` keyword of ``forward``: set for the call, cleared afterwards (also when the call raises)."""
        if n_frames is None:
            yield
            return
        self.set_frame_counts(n_frames)
        try:
            yield
        finally:
            self.set_frame_counts(None)

    def drop_stash(self) -> None:
        """Forget the pending forward (a forward-only call): ``backward`` refuses until the next ``forward``."""
        self._pending = None

    # ---------------------------------------------------------------- forward / backward
    def forward(self, params: Dict[str, torch.Tensor], x_start: torch.Tensor, z: torch.Tensor, t: torch.Tensor, noise: torch.Tensor,
                loss_type: str = "l1", dropout_p: float = 0.0, dropout_sites: int = ALL, seed: int = 0, step: int = 0,
                n_frames=None) -> Dict[str, torch.Tensor]:
        """pd_train_forward: ``{"loss", "x_0_pred", "x_t", "model_out"}`` (each [B, N, 9]) from the live ``params`` (state-dict names ->
        tensors), with the stash one ``backward`` consumes.  ``dropout_p`` > 0: pd_train_forward_dropout at the sites in ``dropout_sites``
        (bits of ``DROPOUT_SITES``) with the masks of ``(seed, step)`` (seed: any int, taken modulo 2^64; step: uint32); ``backward`` then
        differentiates that function.  ``dropout_p == 0`` or ``dropout_sites == 0`` is the call without dropout, bit for bit.
        ``n_frames`` [B]: frame counts per sequence (``set_frame_counts``), set for this call and cleared after it; the stash keeps them
        for ``backward``.  Padding rows of the four outputs are +0; the mean loss over real frames is ``loss.sum() / (9 * sum(n_frames))``."""
        if loss_type not in _LOSS_TYPES:
            raise ValueError(f"invalid loss type {loss_type}")
        if not 0 <= int(step) < 2 ** 32:
            raise ValueError(f"step must fit 32 unsigned bits, got {step}")
        B, N, _ = x_start.shape
        if n_frames is not None:
            n_frames = check_frame_counts(n_frames, B, N)
        live = self._live(params)
        x_start, z, noise = self._f32(x_start, (B, N, 9)), self._f32(z, (B, N, int(self.shape["z_dim"]))), self._f32(noise, (B, N, 9))
        t = torch.as_tensor(t).reshape(-1).to(device=self.device, dtype=torch.int64).contiguous()
        if t.numel() != B:
            raise ValueError(f"expected one timestep per sequence ({B}), got {t.numel()}")
        out = {k: torch.empty_like(x_start) for k in ("loss", "x_0_pred", "x_t", "model_out")}
        w = self._weights_struct(live)
        self._pending = None
        with torch.cuda.device(self.device), self._counts(n_frames):
            outs = (out["loss"].data_ptr(), out["x_0_pred"].data_ptr(), out["x_t"].data_ptr(), out["model_out"].data_ptr(), self._stream())
            ins = (self._h, C.byref(w), x_start.data_ptr(), z.data_ptr(), t.data_ptr(), noise.data_ptr(), B, N, _LOSS_TYPES[loss_type])
            if float(dropout_p) == 0.0 and 0 <= int(dropout_sites) <= ALL:
                _lib.check(self.lib.pd_train_forward(*ins, *outs), "pd_train_forward")
            else:                                # (a bad p or sites is refused by the C entry, which names the argument)
                _lib.check(self.lib.pd_train_forward_dropout(*ins, float(dropout_p), int(dropout_sites) & 0xffffffff, int(seed) % 2 ** 64, int(step),
                                                             *outs), "pd_train_forward_dropout")
        self._generation += 1
        self._pending = self._last_shape = (B, N)
        return out

    def backward(self, params: Dict[str, torch.Tensor], g_loss: torch.Tensor, want: Optional[Iterable[str]] = None) -> Dict[str, torch.Tensor]:
        """pd_train_backward: ``{name: d sum(g_loss * loss) / d param}`` for the names in ``want`` (state-dict names, plus ``"z"``; default:
        every parameter and z).  ``params`` must be the tensors of the forward, unmodified.  A name left out is not computed."""
        if self._pending is None:                # pd_train_backward itself refuses (PD_ERR_STATE): its message is the one raised
            dummy = torch.zeros(1, device=self.device)
            _lib.check(self.lib.pd_train_backward(self._h, C.byref(self._weights_struct(None)), dummy.data_ptr(), C.byref(_lib.pd_weight_grads()),
                                                  None, self._stream()), "pd_train_backward")
            raise RuntimeError("pd_train_backward accepted a call without a pending forward")
        B, N = self._pending
        want = set(self.names + ["z"]) if want is None else set(want)
        unknown = want - set(self.names) - {"z"}
        if unknown:
            raise KeyError(f"unknown gradient names {sorted(unknown)}")
        live = self._live(params)
        g_loss = self._f32(g_loss, (B, N, 9))
        grads = {n: torch.empty_like(live[n]) for n in self.names if n in want}
        if "z" in want:
            grads["z"] = torch.empty(B, N, int(self.shape["z_dim"]), device=self.device)
        g = _lib.pd_weight_grads()
        _fill(g, self.num_layers, lambda n: grads[n].data_ptr() if n in grads else None)
        w = self._weights_struct(live)
        self._pending = None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.pd_train_backward(self._h, C.byref(w), g_loss.data_ptr(), C.byref(g),
                                                  grads["z"].data_ptr() if "z" in grads else None, self._stream()), "pd_train_backward")
        return grads

    def debug_relu(self, layer: int) -> torch.Tensor:
        """pd_train_debug_relu: the stashed post-ReLU activations of encoder layer ``layer`` ([B N, ff]) or, at ``layer == num_layers``, of
        ``_last`` ([B N, hidden]) -- of the last forward."""
        if self._last_shape is None:
            raise RuntimeError("no forward has run on this trainer")
        B, N = self._last_shape
        width = int(self.shape["dim_ff"]) if layer < self.num_layers else int(self.shape["mlp_hidden"])
        out = torch.empty(B * N, width, device=self.device)
        _lib.check(self.lib.pd_train_debug_relu(self._h, int(layer), out.data_ptr(), out.numel(), self._stream()), "pd_train_debug_relu")
        return out


class _PLossesFn(torch.autograd.Function):
    """(trainer, loss_type, x_start, z, t, noise, *params) -> (loss, x_0_pred, x_t, model_out); only ``loss`` is differentiable, with
    respect to the parameters (passed flat so that autograd routes their gradients) and z.  ``loss_type`` is the string, or the tuple
    ``(loss_type, dropout_p, dropout_sites, seed, step[, n_frames])`` of a forward with dropout and / or frame counts."""

    @staticmethod
    def forward(ctx, trainer, loss_type, x_start, z, t, noise, *params):
        sd = dict(zip(trainer.names, params))
        loss_type, *drop = (loss_type,) if isinstance(loss_type, str) else loss_type
        out = trainer.forward(sd, x_start, z, t, noise, loss_type, *drop)
        ctx.trainer, ctx.generation = trainer, trainer._generation
        ctx.z_shape_dtype = (z.shape, z.dtype, z.device)
        ctx.save_for_backward(*params)
        ctx.mark_non_differentiable(out["x_0_pred"], out["x_t"], out["model_out"])
        return out["loss"], out["x_0_pred"], out["x_t"], out["model_out"]

    @staticmethod
    def backward(ctx, g_loss, *_unused):
        tr = ctx.trainer
        if ctx.generation != tr._generation or tr._pending is None:
            raise RuntimeError("PoseTrainer keeps ONE activation stash: backward must follow its own forward, once, before the next forward "
                               "on the same trainer (no retain_graph, no two losses in flight)")
        params = ctx.saved_tensors
        needs = ctx.needs_input_grad
        want = [n for n, need in zip(tr.names, needs[6:]) if need] + (["z"] if needs[3] else [])
        grads = tr.backward(dict(zip(tr.names, params)), g_loss, want)
        gz = grads.get("z")
        if gz is not None:
            shape, dtype, device = ctx.z_shape_dtype
            gz = gz.to(device=device, dtype=dtype).reshape(shape)
        return (None, None, None, gz, None, None) + tuple(grads.get(n) for n in tr.names)


def p_losses_with_grad(trainer: PoseTrainer, denoiser: torch.nn.Module, x_start, z, t, noise, loss_type: str = "l1", dropout_p: float = 0.0,
                       dropout_sites: int = ALL, seed: int = 0, step: int = 0, n_frames=None) -> Dict[str, torch.Tensor]:
    """The p_losses dict of ``trainer.forward`` (same dropout and ``n_frames`` keywords) with ``loss`` attached to ``denoiser``'s
    parameters (and to z when it requires grad).  With ``n_frames`` the gradient of padding rows of z is +0."""
    if n_frames is not None:
        n_frames = check_frame_counts(n_frames, x_start.shape[0], x_start.shape[1])
    named = dict(denoiser.named_parameters())
    params = [named[n] for n in trainer.names]
    mode = loss_type if float(dropout_p) == 0.0 and 0 <= int(dropout_sites) <= ALL else (loss_type, dropout_p, dropout_sites, seed, step)
    if n_frames is not None:
        mode = ((loss_type, 0.0, ALL, 0, 0) if isinstance(mode, str) else mode) + (n_frames,)
    loss, x0, xt, mo = _PLossesFn.apply(trainer, mode, x_start, z, t, noise, *params)
    return {"loss": loss, "x_0_pred": x0, "x_t": xt, "model_out": mo}
