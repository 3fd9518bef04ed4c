"""The optimiser step on the engine (include/pd_engine_optim.h): ``EngineAdamW``, a ``torch.optim.Optimizer`` whose ``step``
is the reference's ``clip_grad_norm_`` + ``torch.optim.AdamW.step()`` (train.py:247-250) in two passes over the live tensors, and
``clip_grad_norm_``, the same norm and scaling for users who keep a PyTorch optimiser.

State lives in ``self.state[p]`` under PyTorch's own keys (``step`` a CPU float tensor, ``exp_avg``, ``exp_avg_sq``) and the groups carry
PyTorch's keys, so ``state_dict`` / ``load_state_dict`` are the base class's, checkpoints pass both ways between ``EngineAdamW`` and
``torch.optim.AdamW``, and any ``torch.optim.lr_scheduler`` drives it.  There is no CPU path and no fallback."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib

CHUNK = _lib.PD_OPTIM_CHUNK   # elements per partial sum of the norm: the granularity at which a tensor is cut into work

_DEFAULT = object()   # step(max_grad_norm=...): the constructor's value
_NO_GPU = "posediffusion_amd.{} needs an AMD GPU (torch.cuda unavailable); there is no CPU fallback"


class _Handle:
    """One pd_optimizer: a table of ``max_tensors`` entries and partial sums for ``max_numel`` elements, on ``device``."""

    def __init__(self, device: torch.device, max_tensors: int, max_numel: int):
        self.lib = _lib.load()
        self.device, self.max_tensors, self.max_numel = device, int(max_tensors), int(max_numel)
        self._h = C.c_void_p(None)
        with torch.cuda.device(device):
            _lib.check(self.lib.pd_optimizer_create(self.max_tensors, self.max_numel, C.byref(self._h)), "pd_optimizer_create")

    def fits(self, n: int, numel: int) -> bool:
        return n <= self.max_tensors and numel <= self.max_numel

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.pd_optimizer_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_live(t: torch.Tensor, what: str, device: torch.device) -> None:
    """The engine reads the live tensor and keeps no copy (PoseTrainer._live's rule): a non-conforming one is an error."""
    if t.is_sparse or t.layout != torch.strided:
        raise ValueError(f"{what} is sparse ({t.layout}): the engine's optimiser takes dense tensors only")
    if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor on {device} (got {t.dtype} on {t.device}, "
                         f"contiguous={t.is_contiguous()}): the engine reads the live tensors and keeps no copy")


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _refuse_capture(who: str) -> None:
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{who} under stream capture: the tensor table of the call would bake this step's pointers into the graph")


# pd_optim_tensor as a numpy record: the table of a step is filled by columns
_TENSOR_DTYPE = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("numel", "<i8"), ("group", "<i4"),
                          ("step", "<i4")])
assert _TENSOR_DTYPE.itemsize == C.sizeof(_lib.pd_optim_tensor)


class _Slot:
    """One parameter of an EngineAdamW and what was checked about it: its state dict, the state's tensors and where everything lies."""
    __slots__ = ("p", "gi", "pi", "st", "m", "v", "step", "ptrs", "numel")

    def __init__(self, p, gi, pi):
        self.p, self.gi, self.pi = p, gi, pi
        self.st = self.m = self.v = self.step = None
        self.ptrs, self.numel = (0, 0, 0), -1

    def bind(self, st, device):
        """(Re)check the parameter and its state `st`, created here as PyTorch creates it when the parameter has none yet."""
        p, what = self.p, f"parameter {self.pi} of group {self.gi}"
        _check_live(p, what, device)
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        for key in ("exp_avg", "exp_avg_sq"):
            _check_live(st[key], f"{key} of {what}", device)
            if st[key].shape != p.shape:
                raise ValueError(f"{key} of {what} has shape {tuple(st[key].shape)}, the parameter {tuple(p.shape)}")
        step = st["step"]
        if not isinstance(step, torch.Tensor) or step.device.type != "cpu" or step.numel() != 1:
            raise ValueError(f"the step count of {what} must be a CPU tensor of one element (PyTorch's default; got {step!r})")
        if step.dim() != 0:
            step = st["step"] = step.reshape(())
        self.st, self.m, self.v, self.step = st, st["exp_avg"], st["exp_avg_sq"], step
        self.ptrs, self.numel = (p.data_ptr(), self.m.data_ptr(), self.v.data_ptr()), p.numel()


class EngineAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` (decoupled weight decay, ``amsgrad=False``, ``maximize=False``) with the reference's global-norm clipping
    folded into the step.  Arguments are ``torch.optim.AdamW``'s plus ``max_grad_norm`` (None: no clipping)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, max_grad_norm=None):
        if isinstance(lr, torch.Tensor):
            raise ValueError("EngineAdamW: lr as a Tensor is not supported (the step's scalars are formed on the host)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm} (None switches clipping off)")
        self.max_grad_norm = max_grad_norm
        self.grad_norm: Optional[torch.Tensor] = None    # 0-dim fp32 device tensor: the norm before clipping of the last step
        self._handle: Optional[_Handle] = None
        self._reset_cache()
        # PyTorch's own group keys, in its order (torch.optim.AdamW is Adam with decoupled_weight_decay=True)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=True)
        super().__init__(params, defaults)

    def _reset_cache(self):
        self.__dict__.update(_slots=None, _slots_key=None, _live=None, _steps=None, _tab=None, _device=None)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._refuse_options(self.param_groups[-1])

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("max_grad_norm", None)
        self.__dict__["grad_norm"] = None
        self.__dict__["_handle"] = None
        self._reset_cache()

    def __getstate__(self):
        state = dict(super().__getstate__())
        state["_handle"] = None
        for key in ("_slots", "_slots_key", "_live", "_steps", "_tab", "_device", "grad_norm"):
            state[key] = None
        return state

    @staticmethod
    def _refuse_options(group) -> None:
        for key in ("amsgrad", "maximize", "capturable", "differentiable"):
            if group.get(key):
                raise ValueError(f"EngineAdamW: {key}=True is not supported (the engine's step is torch.optim.AdamW with amsgrad=False, "
                                 "maximize=False, outside graph capture and autograd)")
        for key in ("foreach", "fused"):
            if group.get(key) is not None:
                raise ValueError(f"EngineAdamW: {key}={group[key]!r} selects one of PyTorch's own implementations; leave it None "
                                 "(the step runs on the engine's kernels)")
        if not group.get("decoupled_weight_decay", True):
            raise ValueError("EngineAdamW: decoupled_weight_decay=False is Adam with L2 regularisation, not AdamW")

    @torch.no_grad()
    def step(self, closure=None, max_grad_norm=_DEFAULT):
        """One step over every parameter that has a gradient (the others keep their ``step``).  ``max_grad_norm``: the constructor's by
        default; None or a value <= 0 switches clipping off for this step.  Asynchronous on the current stream: reading
        ``self.grad_norm`` is the caller's synchronisation, not the step's."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if max_grad_norm is _DEFAULT:
            max_grad_norm = self.max_grad_norm
        for group in self.param_groups:
            self._refuse_options(group)
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_GPU.format("EngineAdamW"))
        _refuse_capture("EngineAdamW.step")

        # the parameters with a gradient, in group order.  A parameter's own tensors are checked when they are first seen and again
        # whenever one of them is another tensor or lies elsewhere than at the last step; its gradient is checked at every step.
        slots = self._slots
        if slots is None or self._slots_key != [len(g["params"]) for g in self.param_groups]:
            slots = self._slots = [_Slot(p, gi, pi) for gi, g in enumerate(self.param_groups) for pi, p in enumerate(g["params"])]
            self._slots_key = [len(g["params"]) for g in self.param_groups]
            self._live = None
        live: List[_Slot] = []
        gptrs: List[int] = []
        device, same, state_of = self._device, True, self.state
        for sl in slots:
            p = sl.p
            g = p.grad
            if g is None:
                continue
            if device is None:
                device = self._device = p.device
                if device.type != "cuda":
                    self._device = None
                    raise ValueError(f"parameter {sl.pi} of group {sl.gi} is on {device}: the engine's optimiser has no CPU path")
            if g.dtype is not torch.float32 or g.layout is not torch.strided or g.device != device or not g.is_contiguous():
                _check_live(g, f"the gradient of parameter {sl.pi} of group {sl.gi}", device)
            st = state_of[p]
            if (st is not sl.st or st.get("exp_avg") is not sl.m or st.get("exp_avg_sq") is not sl.v or st.get("step") is not sl.step
                    or p.data_ptr() != sl.ptrs[0] or sl.m.data_ptr() != sl.ptrs[1] or sl.v.data_ptr() != sl.ptrs[2] or p.numel() != sl.numel):
                sl.bind(st, device)
                same = False
            live.append(sl)
            gptrs.append(g.data_ptr())
        if not live:
            return loss

        n = len(live)
        tab = self._tab
        if tab is None or len(tab) < len(slots):
            tab = self._tab = np.zeros(len(slots), dtype=_TENSOR_DTYPE)
            same = False
        if not same or live != self._live:           # (identity: a _Slot compares by it)
            self._live = live
            self._steps = [sl.step for sl in live]
            tab["param"][:n] = [sl.ptrs[0] for sl in live]
            tab["exp_avg"][:n] = [sl.ptrs[1] for sl in live]
            tab["exp_avg_sq"][:n] = [sl.ptrs[2] for sl in live]
            tab["numel"][:n] = [sl.numel for sl in live]
            tab["group"][:n] = [sl.gi for sl in live]
        steps = self._steps
        tab["grad"][:n] = gptrs
        tab["step"][:n] = torch.stack(steps).to(torch.int32).numpy() + 1
        groups = (_lib.pd_optim_group * len(self.param_groups))()
        for gi, group in enumerate(self.param_groups):
            g = groups[gi]
            g.lr, g.beta1, g.beta2, g.eps, g.weight_decay = (float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]),
                                                              float(group["eps"]), float(group["weight_decay"]))

        n_all, numel_all = len(slots), sum(sl.p.numel() for sl in slots) if self._handle is None or not same else 0
        if self._handle is None or self._handle.device != device or not self._handle.fits(n_all, numel_all):
            if self._handle is not None:             # outgrown by add_param_group
                torch.cuda.synchronize(self._handle.device)
                self._handle.close()
            self._handle = _Handle(device, n_all, max(sum(sl.p.numel() for sl in slots), 1))
        clip = float(max_grad_norm) if max_grad_norm is not None and max_grad_norm > 0 else 0.0
        with torch.cuda.device(device):
            norm = torch.empty((), dtype=torch.float32, device=device)
            _lib.check(self._handle.lib.pd_optim_adamw_step(self._handle._h, tab.ctypes.data_as(C.POINTER(_lib.pd_optim_tensor)), n, groups,
                                                            len(groups), clip, norm.data_ptr(), _stream(device)), "pd_optim_adamw_step")
        self.grad_norm = norm
        torch._foreach_add_(steps, 1.0)              # only now: a refused call leaves every count as it was
        torch.autograd.graph.increment_version([sl.p for sl in live])   # autograd refuses a backward whose forward saw the old values
        return loss


_shared: Dict[torch.device, _Handle] = {}     # clip_grad_norm_ / grad_norm: one handle per device, regrown when a call outgrows it


def _grad_table(parameters, who: str):
    """(table, n, elements, device) of the ``.grad`` of ``parameters`` that are not None."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU.format(who))
    _refuse_capture(who)
    device = grads[0].device if grads else torch.device("cuda", torch.cuda.current_device())
    if device.type != "cuda":
        raise ValueError(f"gradient 0 is on {device}: the engine's {who} has no CPU path")
    tab, numel = (_lib.pd_optim_tensor * max(len(grads), 1))(), 0
    for i, g in enumerate(grads):
        _check_live(g, f"gradient {i}", device)
        tab[i].grad, tab[i].numel = g.data_ptr(), g.numel()
        numel += g.numel()
    return tab, len(grads), numel, device


def _shared_handle(device: torch.device, n: int, numel: int) -> _Handle:
    h = _shared.get(device)
    if h is None or not h.fits(n, numel):
        if h is not None:
            torch.cuda.synchronize(device)
            h.close()
        h = _shared[device] = _Handle(device, max(n, 512), max(numel, 1 << 26))
    return h


def clip_grad_norm_(parameters, max_norm: float) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` for the L2 norm on the engine: scales every ``.grad`` in place by
    ``clamp(max_norm / (norm + 1e-6), max=1)`` and returns the norm before clipping as a 0-dim device tensor (reading it is the caller's
    synchronisation).  A NaN norm makes every gradient NaN and an inf norm zeroes the finite ones, as with ``error_if_nonfinite=False``."""
    tab, n, numel, device = _grad_table(parameters, "clip_grad_norm_")
    h = _shared_handle(device, n, numel)
    with torch.cuda.device(device):
        norm = torch.empty((), dtype=torch.float32, device=device)
        _lib.check(h.lib.pd_optim_clip_grad_norm(h._h, tab, n, float(max_norm), norm.data_ptr(), _stream(device)), "pd_optim_clip_grad_norm")
    return norm


def grad_norm(parameters, capacity: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """The global L2 norm of the ``.grad`` of ``parameters`` (pd_optim_grad_norm) as a 0-dim device tensor; nothing is scaled.
    ``capacity`` = (tensors, elements): through a handle of that capacity of its own (the norm does not depend on it)."""
    tab, n, numel, device = _grad_table(parameters, "grad_norm")
    h = _shared_handle(device, n, numel) if capacity is None else _Handle(device, capacity[0], capacity[1])
    with torch.cuda.device(device):
        norm = torch.empty((), dtype=torch.float32, device=device)
        _lib.check(h.lib.pd_optim_grad_norm(h._h, tab, n, norm.data_ptr(), _stream(device)), "pd_optim_grad_norm")
    if capacity is not None:
        torch.cuda.synchronize(device)
        h.close()
    return norm
