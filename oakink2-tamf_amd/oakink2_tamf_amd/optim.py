"""HipAdamW: torch.optim.AdamW whose step - and the reference's per-parameter gradient clipping in front of it - is two HIP launches
per parameter group (libtamf_optim.so, include/tamf_optim.h), whatever the number of parameters.

The reference runs, after every backward (launch/train.py, launch/train_refine.py, launch/train_encoder.py):
    clip_gradient(optimizer, 0.1, 2.0)     util/net_util.py: one torch.nn.utils.clip_grad_norm_(param, 0.1, 2.0) PER PARAMETER
    optimizer.step()                       torch.optim.AdamW(lr 1e-4, weight_decay 0)
HipAdamW(params, clip_max_norm=0.1).step() is that sequence: each parameter's gradient is scaled by min(1, max_norm / (its own
2-norm + 1e-6)) and fed to torch's single-tensor AdamW arithmetic, in float32.

One difference from the reference: `.grad` is READ, never written.  The reference's clip scales the gradient in place (and its
zero_grad then clears it); here the gradient tensors still hold what backward wrote after the step.

State lives where torch keeps it - self.state[p] = {"step": a CPU float32 scalar tensor, "exp_avg", "exp_avg_sq"}, created at a
parameter's first step with a gradient - so state_dict(), load_state_dict() and the LR schedulers are the inherited ones and an
optimizer_%04d.pt file loads into torch.optim.AdamW and back.  A parameter whose .grad is None, or that has no elements, is skipped
and gets no state, as torch skips it.  No CPU or torch fall-back: without the library or a GPU, step() raises.

Cost of a moved pointer: before each step the data pointers of every p, .grad, exp_avg and exp_avg_sq are compared with the bound
ones, and any change re-binds the table - a synchronisation of the whole device and two blocking host-to-device copies
(tamf_optim_bind).  With gradient buffers that stay where they are (the native training steps re-attach theirs after zero_grad()) a
step synchronises nothing.  The usual `zero_grad()` + backward into freshly allocated .grad tensors pays that synchronisation inside
every step(): keep the gradients in place (`zero_grad(set_to_none=False)`) where the step's latency matters."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_char_p, c_double, c_int32, c_int64, c_void_p
from typing import List, Optional

import torch

_bound = None
_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable", "fused")


def _bind():
    global _bound
    if _bound is None:
        from . import _lib

        L = _lib.load_optim()
        L.tamf_optim_last_error.restype = c_char_p
        L.tamf_optim_last_error.argtypes = []
        L.tamf_optim_create.argtypes = [c_int32, POINTER(c_void_p)]
        L.tamf_optim_destroy.argtypes = [c_void_p]
        L.tamf_optim_destroy.restype = None
        L.tamf_optim_bind.argtypes = [c_void_p, c_int32] + [POINTER(c_void_p)] * 4 + [POINTER(c_int64)]
        L.tamf_optim_grad_norms.argtypes = [c_void_p, c_void_p, c_void_p]
        L.tamf_optim_step.argtypes = [c_void_p] + [c_double] * 6 + [c_int64, c_void_p]
        _bound = L
    return _bound


def _check(L, rc: int) -> None:
    if rc != 0:
        from .hip_backend import TamfError

        msg = L.tamf_optim_last_error()
        raise TamfError(f"libtamf_optim error {rc}: {msg.decode() if msg else '?'}")


def table_key(tensors):
    """the data pointers and sizes of [(p, g, exp_avg, exp_avg_sq)]; a tensor without state yet has None for the last two"""
    return tuple((p.data_ptr(), g.data_ptr(), 0 if m is None else m.data_ptr(), 0 if v is None else v.data_ptr(), p.numel()) for p, g, m, v in tensors)


class _Table:
    """One native context: the tensor table of one set of parameters that step together, bound where the tensors live now"""

    def __init__(self, device: torch.device):
        self.L = _bind()
        self.device = device
        self.key = None  # the data pointers and sizes of the bound table
        self.host = None  # the host arrays of the last bind: kept until the next one
        h = c_void_p()
        _check(self.L, self.L.tamf_optim_create(device.index or 0, ctypes.byref(h)))
        self.h = h

    def ensure(self, tensors) -> None:
        """bind [(p, g, exp_avg, exp_avg_sq)] unless exactly these addresses are bound already"""
        key = table_key(tensors)
        if key == self.key:
            return
        n = len(key)
        cols = [(c_void_p * n)(*[row[j] for row in key]) for j in range(4)]
        numel = (c_int64 * n)(*[row[4] for row in key])
        self.key = None
        self.host = (cols, numel)
        _check(self.L, self.L.tamf_optim_bind(self.h, n, *cols, numel))
        self.key = key

    def close(self) -> None:
        if self.h is not None and self.h.value:
            self.L.tamf_optim_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _refuse_param(p: torch.Tensor, where: str) -> None:
    if p.dtype != torch.float32:
        raise ValueError(f"HipAdamW: {where} is {p.dtype}; the native step takes float32 parameters only")
    if p.is_sparse or not p.is_contiguous():
        raise ValueError(f"HipAdamW: {where} of shape {tuple(p.shape)} is not contiguous; the native step takes contiguous parameters only")


class HipAdamW(torch.optim.AdamW):
    """torch.optim.AdamW(params, lr, betas, eps, weight_decay) with the step in HIP; clip_max_norm=c additionally clips every
    parameter's gradient to the 2-norm c ON ITS OWN before the update (None: no clipping).  ValueError for amsgrad, maximize,
    capturable, differentiable, fused, a tensor lr, and parameters that are not contiguous float32."""

    def __init__(self, params, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 clip_max_norm: Optional[float] = None, **kwargs):
        for name in _UNSUPPORTED:
            if kwargs.pop(name, False):
                raise ValueError(f"HipAdamW: {name}=True is not supported by the native step")
        if kwargs.pop("foreach", None):
            raise ValueError("HipAdamW: foreach=True is not supported: the native step is one call per parameter group")
        if kwargs:
            raise TypeError(f"HipAdamW: unexpected arguments {sorted(kwargs)}")
        if isinstance(lr, torch.Tensor):
            raise ValueError("HipAdamW: a tensor lr is not supported: lr is a host scalar of the native step")
        if clip_max_norm is not None and not float(clip_max_norm) >= 0.0:
            raise ValueError(f"HipAdamW: clip_max_norm = {clip_max_norm} must be None or >= 0")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        for gi, group in enumerate(self.param_groups):
            for pi, p in enumerate(group["params"]):
                _refuse_param(p, f"parameter {pi} of group {gi}")
        self.clip_max_norm = None if clip_max_norm is None else float(clip_max_norm)
        self._tables = {}  # (group index, rank of the step count in the group - or "norms", grad_norms' own) -> _Table

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for pi, p in enumerate(self.param_groups[-1]["params"]):
            _refuse_param(p, f"parameter {pi} of group {len(self.param_groups) - 1}")

    def _active(self, group, gi: int, create_state: bool = True) -> List:
        """[(p, grad, state)] of the group's parameters that take part in a step.  create_state: a parameter without state gets it
        as torch creates it, at its first step(); otherwise its state is None here and stays absent"""
        for name in _UNSUPPORTED:
            if group.get(name, False):
                raise ValueError(f"HipAdamW: {name}=True (param group {gi}) is not supported by the native step")
        if isinstance(group["lr"], torch.Tensor):
            raise ValueError("HipAdamW: a tensor lr is not supported: lr is a host scalar of the native step")
        rows = []
        for pi, p in enumerate(group["params"]):
            g = p.grad
            if g is None or p.numel() == 0:
                continue
            _refuse_param(p, f"parameter {pi} of group {gi}")
            if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or g.device != p.device:
                raise ValueError(f"HipAdamW: the gradient of parameter {pi} of group {gi} must be dense contiguous float32 of the parameter's shape "
                                 f"and device, got {g.dtype} {tuple(g.shape)} on {g.device}")
            st = self.state[p] if create_state else self.state.get(p)
            if st is not None and len(st) == 0:
                if create_state:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                else:
                    st = None
            for k in ("exp_avg", "exp_avg_sq") if st is not None else ():
                if st[k].dtype != torch.float32 or not st[k].is_contiguous() or st[k].device != p.device or st[k].shape != p.shape:
                    raise ValueError(f"HipAdamW: state {k} of parameter {pi} of group {gi} must be contiguous float32 on the parameter's device")
            rows.append((p, g, st))
        return rows

    @staticmethod
    def _tensors(rows):
        return [(p.data, g, None if st is None else st["exp_avg"], None if st is None else st["exp_avg_sq"]) for p, g, st in rows]

    def _table(self, gi: int, rank, rows) -> _Table:
        from .hip_backend import require_gpu

        dev = require_gpu(rows[0][0].device)
        for p, _, _ in rows:
            if p.device != dev:
                raise ValueError(f"HipAdamW: the parameters of group {gi} live on {dev} and {p.device}; one device per group")
        tab = self._tables.get((gi, rank))
        if tab is None or tab.device != dev:
            if tab is not None:
                tab.close()
            tab = self._tables[(gi, rank)] = _Table(dev)
        tab.ensure(self._tensors(rows))
        return tab

    @torch.no_grad()
    def step(self, closure=None):
        from .hip_backend import _stream_ptr

        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            rows = self._active(group, gi)
            if not rows:
                continue
            # the parameters of a group normally share one step count; those that do not (a gradient that was None for some steps)
            # go through a table of their own per count, since the bias corrections are the call's
            taken = [int(st["step"]) for _, _, st in rows]
            counts = sorted(set(taken))
            parts = [rows] if len(counts) == 1 else [[r for r, t in zip(rows, taken) if t == count] for count in counts]  # (before any counter moves)
            beta1, beta2 = group["betas"]
            for rank, (count, part) in enumerate(zip(counts, parts)):
                tab = self._table(gi, rank, part)
                with torch.cuda.device(tab.device):
                    _check(tab.L, tab.L.tamf_optim_step(tab.h, float(group["lr"]), float(beta1), float(beta2), float(group["eps"]),
                                                        float(group["weight_decay"]), -1.0 if self.clip_max_norm is None else self.clip_max_norm,
                                                        count + 1, c_void_p(_stream_ptr(tab.device))))
                for _, _, st in part:  # (after the call: a refused step leaves the counters where they were)
                    st["step"] += 1
        return loss

    @torch.no_grad()
    def grad_norms(self) -> torch.Tensor:
        """The 2-norm of every parameter's gradient, one float32 per parameter in param_groups order (0 where .grad is None or the
        parameter is empty), as a device tensor; nothing is copied to the host.  What the clip of the next step() will see.
        Creates no optimiser state.  Runs on the table step() bound when that holds exactly these tensors (one step count in the group,
        state present), otherwise on a table of its own, so the two calls never re-bind each other's."""
        from .hip_backend import _stream_ptr, require_gpu

        outs = []
        for gi, group in enumerate(self.param_groups):
            params = group["params"]
            rows = self._active(group, gi, create_state=False)
            if not rows:
                dev = require_gpu(params[0].device) if params else require_gpu()
                outs.append(torch.zeros(len(params), dtype=torch.float32, device=dev))
                continue
            shared = self._tables.get((gi, 0))
            tab = shared if shared is not None and shared.key == table_key(self._tensors(rows)) else self._table(gi, "norms", rows)
            part = torch.empty(len(rows), dtype=torch.float32, device=tab.device)
            with torch.cuda.device(tab.device):
                _check(tab.L, tab.L.tamf_optim_grad_norms(tab.h, c_void_p(part.data_ptr()), c_void_p(_stream_ptr(tab.device))))
            if len(rows) == len(params):
                outs.append(part)
            else:
                where = {id(p): i for i, p in enumerate(params)}
                full = torch.zeros(len(params), dtype=torch.float32, device=tab.device)
                full[torch.tensor([where[id(p)] for p, _, _ in rows], device=tab.device)] = part
                outs.append(full)
        return torch.cat(outs) if outs else torch.zeros(0, dtype=torch.float32)

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("_tables", {})  # (native contexts are per process and never pickled)
        self.__dict__.setdefault("clip_max_norm", None)

    def close(self) -> None:
        """release the native contexts (they are rebuilt by the next step)"""
        for tab in self._tables.values():
            tab.close()
        self._tables = {}


__all__ = ["HipAdamW"]
