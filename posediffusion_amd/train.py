"""PoseTrainer: thin Python owner of a ``pd_trainer`` (include/pd_engine_train.h) -- the diffusion loss of
GaussianDiffusion.p_losses (models/gaussian_diffuser.py:308-327) and its gradient with respect to every Denoiser parameter (and z),
computed by hand-written gfx950 kernels from the LIVE PyTorch parameters: an optimiser step needs no rebuild and no repacking.

PyTorch keeps the optimiser, the LR schedule and gradient clipping (the reference's train.py:73-77, 245-251); ``p_losses_with_grad``
is the ``torch.autograd.Function`` that hands the engine's gradients to autograd.  Exact fp32, pre-norm only, head dim <= 128, N <= 64
frames by default and up to 256 with ``max_frames`` / ``set_max_frames`` (PD_TR_OPT_MAX_FRAMES): above 64 frames the attention runs
key-tiled kernels, which at N <= 64 give the bits of the default ones (``set_long_attn``, for the tests).
Without ``dropout_p`` it is the eval-mode function; with it, the ``.train()``-mode one: dropout at the four sites of every encoder layer
(``DROPOUT_SITES``), masks from Philox4x32-10 keyed by ``(seed, step)`` and recomputed by the backward (pd_train_forward_dropout).
``backward(..., g_model_out=, g_x0_pred=)`` / ``p_losses_with_grad(..., differentiable_outputs=True)``: the prediction is differentiable
too, as the reference's ``p_losses`` returns it -- upstream gradients of ``model_out`` and ``x_0_pred`` enter the backward beside the
loss's (pd_train_backward_ex), and ``pose_to_camera_with_grad`` differentiates the decode of ``x_0_pred`` into cameras
(pd_pose_to_camera_backward), so a camera-space loss term reaches the denoiser's parameters and z.
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

    def backward(self, params: Dict[str, torch.Tensor], g_loss: Optional[torch.Tensor] = None, want: Optional[Iterable[str]] = None,
                 g_model_out: Optional[torch.Tensor] = None, g_x0_pred: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """``{name: dS / d param}`` for the names in ``want`` (state-dict names, plus ``"z"``; default: every parameter and z), with
        S = sum(g_loss * loss) + sum(g_model_out * model_out) + sum(g_x0_pred * x_0_pred); an upstream left ``None`` is absent (a NULL
        pointer, not zeros).  ``g_loss`` alone is pd_train_backward, anything else pd_train_backward_ex.  ``params`` must be the tensors
        of the forward, unmodified.  A name left out is not computed."""
        ex = g_model_out is not None or g_x0_pred is not None or g_loss is None
        if self._pending is None:                # the C entry itself refuses (PD_ERR_STATE): its message is the one raised
            dummy = torch.zeros(1, device=self.device)
            _lib.check(self.lib.pd_train_backward(self._h, C.byref(self._weights_struct(None)), dummy.data_ptr(), C.byref(_lib.pd_weight_grads()),
                                                  None, self._stream()), "pd_train_backward")
            raise RuntimeError("pd_train_backward accepted a call without a pending forward")
        if g_loss is None and g_model_out is None and g_x0_pred is None:      # refused by the C entry (PD_ERR_INVALID_ARG); the stash stays
            _lib.check(self.lib.pd_train_backward_ex(self._h, C.byref(self._weights_struct(None)), None, None, None,
                                                     C.byref(_lib.pd_weight_grads()), None, self._stream()), "pd_train_backward_ex")
            raise RuntimeError("pd_train_backward_ex accepted a call without an upstream gradient")
        B, N = self._pending
        want = set(self.names + ["z"]) if want is None else set(want)
        unknown = want - set(self.names) - {"z"}
        if unknown:
            raise KeyError(f"unknown gradient names {sorted(unknown)}")
        live = self._live(params)
        g_loss, g_model_out, g_x0_pred = (None if g is None else self._f32(g, (B, N, 9)) for g in (g_loss, g_model_out, g_x0_pred))
        grads = {n: torch.empty_like(live[n]) for n in self.names if n in want}
        if "z" in want:
            grads["z"] = torch.empty(B, N, int(self.shape["z_dim"]), device=self.device)
        g = _lib.pd_weight_grads()
        _fill(g, self.num_layers, lambda n: grads[n].data_ptr() if n in grads else None)
        w = self._weights_struct(live)
        self._pending = None
        dz = grads["z"].data_ptr() if "z" in grads else None
        with torch.cuda.device(self.device):
            if not ex:
                _lib.check(self.lib.pd_train_backward(self._h, C.byref(w), g_loss.data_ptr(), C.byref(g), dz, self._stream()), "pd_train_backward")
            else:
                rc = self.lib.pd_train_backward_ex(self._h, C.byref(w), *(None if u is None else u.data_ptr() for u in (g_loss, g_model_out, g_x0_pred)),
                                                   C.byref(g), dz, self._stream())
                if rc == -4 and "g_x0_pred" in _lib.last_error():      # refused for the missing recip tables: nothing ran, the stash is still pending
                    self._pending = (B, N)
                _lib.check(rc, "pd_train_backward_ex")
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
    """(trainer, loss_type, x_start, z, t, noise, *params) -> (loss, x_0_pred, x_t, model_out), differentiable with respect to the
    parameters (passed flat so that autograd routes their gradients) and z.  ``loss_type`` is the string, or the tuple
    ``(loss_type, dropout_p, dropout_sites, seed, step[, n_frames[, differentiable_outputs]])`` of a forward with dropout, frame counts
    and / or differentiable outputs.  By default only ``loss`` is differentiable.  With ``differentiable_outputs`` so are ``x_0_pred``
    and ``model_out`` (``x_t`` stays data), and undefined upstream gradients are NOT materialised: an output nobody used reaches
    pd_train_backward_ex as a NULL pointer, not as a tensor of zeros."""

    @staticmethod
    def forward(ctx, trainer, loss_type, x_start, z, t, noise, *params):
        sd = dict(zip(trainer.names, params))
        loss_type, *drop = (loss_type,) if isinstance(loss_type, str) else loss_type
        ctx.outputs = bool(drop.pop()) if len(drop) == 6 else False
        out = trainer.forward(sd, x_start, z, t, noise, loss_type, *drop)
        ctx.trainer, ctx.generation = trainer, trainer._generation
        ctx.z_shape_dtype = (z.shape, z.dtype, z.device)
        ctx.save_for_backward(*params)
        if ctx.outputs:
            ctx.set_materialize_grads(False)
            ctx.mark_non_differentiable(out["x_t"])
        else:
            ctx.mark_non_differentiable(out["x_0_pred"], out["x_t"], out["model_out"])
        return out["loss"], out["x_0_pred"], out["x_t"], out["model_out"]

    @staticmethod
    def backward(ctx, g_loss, g_x0_pred=None, _g_xt=None, g_model_out=None):
        tr = ctx.trainer
        n_in = 6 + len(tr.names)
        if not ctx.outputs:
            g_x0_pred = g_model_out = None
        elif g_loss is None and g_x0_pred is None and g_model_out is None:      # nothing flows back: the stash is left alone
            return (None,) * n_in
        if ctx.generation != tr._generation or tr._pending is None:
            raise RuntimeError("PoseTrainer keeps ONE activation stash: backward must follow its own forward, once, before the next forward "
                               "on the same trainer (no retain_graph, no two losses in flight)")
        params = ctx.saved_tensors
        needs = ctx.needs_input_grad
        want = [n for n, need in zip(tr.names, needs[6:]) if need] + (["z"] if needs[3] else [])
        grads = tr.backward(dict(zip(tr.names, params)), g_loss, want, g_model_out=g_model_out, g_x0_pred=g_x0_pred)
        gz = grads.get("z")
        if gz is not None:
            shape, dtype, device = ctx.z_shape_dtype
            gz = gz.to(device=device, dtype=dtype).reshape(shape)
        return (None, None, None, gz, None, None) + tuple(grads.get(n) for n in tr.names)


def p_losses_with_grad(trainer: PoseTrainer, denoiser: torch.nn.Module, x_start, z, t, noise, loss_type: str = "l1", dropout_p: float = 0.0,
                       dropout_sites: int = ALL, seed: int = 0, step: int = 0, n_frames=None,
                       differentiable_outputs: bool = False) -> Dict[str, torch.Tensor]:
    """The p_losses dict of ``trainer.forward`` (same dropout and ``n_frames`` keywords) with ``loss`` attached to ``denoiser``'s
    parameters (and to z when it requires grad).  With ``n_frames`` the gradient of padding rows of z is +0.
    ``differentiable_outputs``: ``x_0_pred`` and ``model_out`` are attached too, so any loss written on them (or on cameras decoded from
    ``x_0_pred``) flows back through pd_train_backward_ex; ``x_t`` stays data.  Still ONE stash: every term must be part of the one
    total whose ``.backward()`` follows this forward (no ``retain_graph``)."""
    if n_frames is not None:
        n_frames = check_frame_counts(n_frames, x_start.shape[0], x_start.shape[1])
    named = dict(denoiser.named_parameters())
    params = [named[n] for n in trainer.names]
    mode = loss_type if float(dropout_p) == 0.0 and 0 <= int(dropout_sites) <= ALL else (loss_type, dropout_p, dropout_sites, seed, step)
    if n_frames is not None or differentiable_outputs:
        mode = ((loss_type, 0.0, ALL, 0, 0) if isinstance(mode, str) else mode) + (n_frames,)
    if differentiable_outputs:
        mode = mode + (True,)
    loss, x0, xt, mo = _PLossesFn.apply(trainer, mode, x_start, z, t, noise, *params)
    return {"loss": loss, "x_0_pred": x0, "x_t": xt, "model_out": mo}


class _PoseToCameraFn(torch.autograd.Function):
    """pose_encoding_to_camera with a gradient: (enc [n, 9], bias, min, max, engine) -> (R [n, 3, 3], T [n, 3], focal [n, 2]) by
    pd_pose_to_camera_ex, backward by pd_pose_to_camera_backward (which recomputes the decode from ``enc``).  Undefined upstream
    gradients are not materialised: an output nobody used is a NULL pointer."""

    @staticmethod
    def forward(ctx, enc, bias, fmin, fmax, engine):
        enc32 = enc.detach().to(device=engine.device, dtype=torch.float32).reshape(-1, 9).contiguous()
        R, T, f = engine.pose_to_camera(enc32, bias, fmin, fmax)
        ctx.save_for_backward(enc32)
        ctx.args = (float(bias), float(fmin), float(fmax), enc.shape, enc.dtype, enc.device)
        ctx.set_materialize_grads(False)
        return R, T, f

    @staticmethod
    def backward(ctx, g_R, g_T, g_f):
        if g_R is None and g_T is None and g_f is None:
            return None, None, None, None, None
        enc32, = ctx.saved_tensors
        bias, fmin, fmax, shape, dtype, device = ctx.args
        n = enc32.shape[0]
        ups = [None if g is None else g.detach().to(device=enc32.device, dtype=torch.float32).reshape(n, w).contiguous()
               for g, w in ((g_R, 9), (g_T, 3), (g_f, 2))]
        out = torch.empty_like(enc32)
        with torch.cuda.device(enc32.device):
            _lib.check(_lib.load().pd_pose_to_camera_backward(enc32.data_ptr(), *(None if u is None else u.data_ptr() for u in ups), n, bias, fmin,
                                                              fmax, out.data_ptr(), torch.cuda.current_stream(enc32.device).cuda_stream),
                       "pd_pose_to_camera_backward")
        return out.reshape(shape).to(device=device, dtype=dtype), None, None, None, None


def pose_to_camera_with_grad(engine, enc, log_focal_length_bias: float = 1.8, min_focal_length: float = 0.1, max_focal_length: float = 20.0):
    """(R, T, focal_length) of ``engine.pose_to_camera`` attached to ``enc`` (the drop-in's pose_encoding_to_camera uses it when grad mode
    is on and ``enc`` requires grad)."""
    return _PoseToCameraFn.apply(enc, log_focal_length_bias, min_focal_length, max_focal_length, engine)
