"""What the two native training steps share (SegmentEncoderTrainStep on libtamf_enctrain.so, SegmentRefineTrainStep on
libtamf_refinetrain.so): the typing and the error check of the entry points both libraries have, under their symbol prefix
(tamf_enctrain_ / tamf_refinetrain_), the dropout keep-mask, the clip-id vector, and TrainStep - the context handle with the binding of
a module's tensors where torch keeps them."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_char_p, c_float, c_int32, c_int64, c_uint32, c_uint64, c_void_p
from typing import Mapping, Optional, Sequence

import numpy as np
import torch

from ..hip_backend import TamfError, _Arch, _stream_ptr, require_gpu

_typed = set()  # library objects whose argtypes are set


def typed_lib(load, prefix: str, own: Mapping[str, list]) -> ctypes.CDLL:
    """load() with the argtypes of <prefix>last_error, create, destroy, bind and dropout_mask, and of the library's `own` entry points"""
    L = load()
    if id(L) not in _typed:
        f = {name: getattr(L, prefix + name) for name in ("last_error", "create", "destroy", "bind", "dropout_mask", *own)}
        f["last_error"].restype = c_char_p
        f["last_error"].argtypes = []
        f["create"].argtypes = [POINTER(_Arch), c_int32, c_int32, c_int32, POINTER(c_void_p)]
        f["destroy"].argtypes = [c_void_p]
        f["destroy"].restype = None
        f["bind"].argtypes = [c_void_p, c_char_p, c_void_p, c_void_p, POINTER(c_int64), c_int32]
        f["dropout_mask"].argtypes = [c_uint64, c_uint32, c_int64, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p]
        for name, argtypes in own.items():
            f[name].argtypes = argtypes
        _typed.add(id(L))
    return L


def check(L: ctypes.CDLL, prefix: str, rc: int) -> None:
    if rc != 0:
        msg = getattr(L, prefix + "last_error")()
        raise TamfError(f"lib{prefix.rstrip('_')} error {rc}: {msg.decode() if msg else '?'}")


def dropout_mask(L: ctypes.CDLL, prefix: str, seed: int, step: int, clip_id: int, site: int, rows: int, cols: int, p: float, device=None) -> torch.Tensor:
    """the (rows, cols) bool keep-mask of one dropout site of one clip (<prefix>dropout_mask)"""
    dev = require_gpu(device)
    out = torch.empty(int(rows), int(cols), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(L, prefix, getattr(L, prefix + "dropout_mask")(int(seed), int(step), int(clip_id), int(site), int(rows), int(cols), float(p),
                                                             c_void_p(out.data_ptr()), c_void_p(_stream_ptr(dev))))
    return out.bool()


def clip_id_vector(clip_ids, B: int) -> Optional[np.ndarray]:
    """clip_ids as an int64 vector of B ids, or None; ValueError for another shape"""
    if clip_ids is None:
        return None
    clip_np = np.ascontiguousarray(torch.as_tensor(clip_ids).cpu().numpy() if isinstance(clip_ids, torch.Tensor) else clip_ids, dtype=np.int64)
    if clip_np.shape != (B,):
        raise ValueError(f"clip_ids must hold one id per clip: shape {clip_np.shape} for B = {B}")
    return clip_np


class TrainStep:
    """A context of one training library around `model` on a GPU.  A subclass names its library: LIB (the module's lib), PREFIX and
    BUFFERS (the buffers of the module that the library declares)."""

    LIB = PREFIX = None
    BUFFERS: Sequence[str] = ()
    _h = None  # (close() works on an object whose __init__ raised before the context was created)

    def __init__(self, model, arch: _Arch, max_batch: int, max_frames: int, dropout: float, seed: int):
        self.model = model
        self.dropout = dropout
        self.seed = int(seed)
        self.max_batch, self.max_frames = int(max_batch), int(max_frames)
        self.device = require_gpu(next(model.parameters()).device)
        self._L = self.LIB()
        h = c_void_p()
        with torch.cuda.device(self.device):
            self._call("create", ctypes.byref(arch), self.max_batch, self.max_frames, self.device.index or 0, ctypes.byref(h))
        self._h = h
        self._bound = {}
        try:
            self.bind()
        except Exception:
            self.close()
            raise

    def _call(self, name: str, *args) -> None:
        """<PREFIX><name>(*args); TamfError with the library's message unless it returns 0"""
        check(self._L, self.PREFIX, getattr(self._L, self.PREFIX + name)(*args))

    def _require_open(self) -> None:
        if self._h is None:
            raise TamfError("the training step is closed")

    def bind(self, skip: Sequence[str] = ()) -> None:
        """(Re)bind every tensor of the module where it lives now: call again after anything that moves the parameters (model.to,
        load_state_dict keeps them in place and needs no call).  `skip` leaves names unbound (for the tests of the refusals)."""
        for name, p in self.model.named_parameters():
            if not p.is_contiguous() or p.dtype != torch.float32:
                raise TamfError(f"{name}: parameters must be contiguous float32")
            p.requires_grad_(True)
            if p.grad is None or p.grad.shape != p.shape or not p.grad.is_contiguous():
                p.grad = torch.zeros_like(p)
            if name not in skip:
                self._bind_one(name, p.data, p.grad)
        for name, b in self.model.named_buffers():
            if name in self.BUFFERS and name not in skip:
                self._bind_one(name, b, None)

    def _rebind_moved(self) -> None:
        """Before every step: a parameter whose .grad is None again (optimizer.zero_grad() sets it to None by default) gets its bound
        gradient tensor back - the step overwrites every element anyway; a parameter or gradient that lives elsewhere than at the
        bind (model.to, an assigned .grad) is bound again where it is now.  So the kernels never write into a tensor the optimiser
        does not see."""
        for name, p in self.model.named_parameters():
            t, g = self._bound.get(name, (None, None))
            if t is None:
                continue  # (left unbound on purpose: the step reports it)
            if p.grad is None and g is not None and g.shape == p.shape and g.device == p.device:
                p.requires_grad_(True)
                p.grad = g
            if p.grad is None or p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or p.grad.shape != p.shape:
                p.requires_grad_(True)
                p.grad = torch.zeros_like(p)
            if p.data_ptr() != t.data_ptr() or p.grad.data_ptr() != g.data_ptr():
                if not p.is_contiguous() or p.dtype != torch.float32:
                    raise TamfError(f"{name}: parameters must be contiguous float32")
                self._bind_one(name, p.data, p.grad)
        for name, b in self.model.named_buffers():
            if name in self._bound and b.data_ptr() != self._bound[name][0].data_ptr():
                self._bind_one(name, b, None)

    def _bind_one(self, name: str, t: torch.Tensor, g: Optional[torch.Tensor]) -> None:
        shape = (c_int64 * t.dim())(*t.shape)
        self._call("bind", self._h, name.encode(), c_void_p(t.data_ptr()), c_void_p(g.data_ptr() if g is not None else 0), shape, t.dim())
        self._bound[name] = (t, g)

    def close(self) -> None:
        if self._h is not None and self._h.value:
            torch.cuda.synchronize(self.device)
            getattr(self._L, self.PREFIX + "destroy")(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
