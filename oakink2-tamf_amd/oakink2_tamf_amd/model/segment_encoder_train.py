"""SegmentEncoderTrainStep - one training step of the FID score's SegmentEncoder on the gfx950 HIP library libtamf_enctrain.so
(include/tamf_enctrain.h): the training-mode forward, the cross-entropy of SegmentEncoderLoss and the gradient of every parameter.

The kernels read the module's parameters where torch keeps them and write into the parameters' .grad tensors, overwriting them: any
torch.optim optimiser then steps on the device.  There is no PyTorch compute path and no fallback.  After optimiser steps call
model.refresh_hip_weights() before using the inference path (SegmentEncoder.forward / encode).

Dropout masks are Philox draws keyed by (seed, step, clip id, site, element): see the header for the sites.  dropout_mask() returns
the keep-mask the step uses at one site, so that a run can be reproduced or checked elsewhere.
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_char_p, c_float, c_int32, c_int64, c_uint32, c_uint64, c_void_p
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from ..hip_backend import TamfError, _Arch, _stream_ptr, encoder_batch, require_gpu

BUFFERS = ("classification_token", "hand_side_process.rh_embed", "hand_side_process.lh_embed", "sequence_pos_encoder.pe")

_typed = set()  # library objects whose argtypes are set


def lib() -> ctypes.CDLL:
    L = _lib.load_enctrain()
    if id(L) not in _typed:
        L.tamf_enctrain_last_error.restype = c_char_p
        L.tamf_enctrain_last_error.argtypes = []
        L.tamf_enctrain_create.argtypes = [POINTER(_Arch), c_int32, c_int32, c_int32, POINTER(c_void_p)]
        L.tamf_enctrain_destroy.argtypes = [c_void_p]
        L.tamf_enctrain_destroy.restype = None
        L.tamf_enctrain_bind.argtypes = [c_void_p, c_char_p, c_void_p, c_void_p, POINTER(c_int64), c_int32]
        L.tamf_enctrain_step.argtypes = [c_void_p, c_int32, c_int32, c_int32] + [c_void_p] * 8 + [c_float, c_uint64, c_uint32, c_void_p, c_void_p, c_void_p]
        L.tamf_enctrain_dropout_mask.argtypes = [c_uint64, c_uint32, c_int64, c_int32, c_int32, c_int32, c_float, c_void_p, c_void_p]
        _typed.add(id(L))
    return L


def _check(rc: int) -> None:
    if rc != 0:
        msg = lib().tamf_enctrain_last_error()
        raise TamfError(f"libtamf_enctrain error {rc}: {msg.decode() if msg else '?'}")


def check_labels(labels, input_dim: int) -> np.ndarray:
    """labels as an int64 vector; ValueError unless every one is in [0, input_dim): the output head has input_dim logits
    (reference model/segment_encoder.py:73)"""
    lab = np.ascontiguousarray(labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else labels)
    if lab.ndim != 1 or (lab.size and not np.issubdtype(lab.dtype, np.integer)):
        raise ValueError(f"labels must be a vector of integers, got shape {lab.shape} of {lab.dtype}")
    lab = lab.astype(np.int64)
    if lab.size and (lab.min() < 0 or lab.max() >= int(input_dim)):
        raise ValueError(f"labels must be in [0, input_dim = {int(input_dim)}): the output head has input_dim logits; got "
                         f"[{int(lab.min())}, {int(lab.max())}]")
    return lab


def dropout_mask(seed: int, step: int, clip_id: int, site: int, rows: int, cols: int, p: float, device=None) -> torch.Tensor:
    """the (rows, cols) bool keep-mask of one dropout site of one clip (tamf_enctrain_dropout_mask)"""
    dev = require_gpu(device)
    out = torch.empty(int(rows), int(cols), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib().tamf_enctrain_dropout_mask(int(seed), int(step), int(clip_id), int(site), int(rows), int(cols), float(p),
                                                c_void_p(out.data_ptr()), c_void_p(_stream_ptr(dev))))
    return out.bool()


class SegmentEncoderTrainStep:
    """loss_and_grads(batch, labels) around a SegmentEncoder on a GPU.  Enables requires_grad on the trainable parameters (all of
    nn.Module.parameters(); the classification token, the hand-side embeddings and the PE table are buffers) and allocates their
    .grad.  dropout=None takes model.dropout."""

    def __init__(self, model, max_batch: int, max_frames: int, dropout: Optional[float] = None, seed: int = 0):
        self.model = model
        self._h = None
        self.dropout = float(model.dropout if dropout is None else dropout)
        self.seed = int(seed)
        self.max_batch, self.max_frames = int(max_batch), int(max_frames)
        self.device = require_gpu(next(model.parameters()).device)
        self.input_dim = int(model.input_feats)
        a = model._arch
        arch = _Arch(a["input_dim"], a["obj_input_dim"], a["hand_shape_dim"], a["obj_embed_dim"], a["latent_dim"], a["ff_size"], a["num_layers"],
                     a["num_heads"], 0, 0, 2)
        self._L = lib()
        h = c_void_p()
        with torch.cuda.device(self.device):
            _check(self._L.tamf_enctrain_create(ctypes.byref(arch), self.max_batch, self.max_frames, self.device.index or 0, ctypes.byref(h)))
        self._h = h
        self._bound = {}
        try:
            self.bind()
        except Exception:
            self.close()
            raise

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
            if name in BUFFERS and name not in skip:
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
        _check(self._L.tamf_enctrain_bind(self._h, name.encode(), c_void_p(t.data_ptr()), c_void_p(g.data_ptr() if g is not None else 0), shape, t.dim()))
        self._bound[name] = (t, g)

    def close(self) -> None:
        if self._h is not None and self._h.value:
            torch.cuda.synchronize(self.device)
            self._L.tamf_enctrain_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def loss_and_grads(self, batch: Dict, labels, obj_num: Optional[Sequence[int]] = None, clip_ids: Optional[Sequence[int]] = None,
                       step: int = 0) -> Dict:
        """batch: "pose_repr" (B, T, input_dim), "hand_side" (B x "rh"/"lh"), "shape" (B, T, 10), "obj_embedding" (B, nobj, od),
        "obj_traj" (B, nobj, T, 9); labels (B,) integers in [0, input_dim) - the output head has input_dim logits.
        Fills p.grad of every trainable parameter (overwriting) -> {"loss", "ce", "acc", "activation"} (device tensors).
        optimizer.zero_grad() between steps is harmless and unnecessary: gradients set to None get their tensors back, and tensors
        that moved are bound again (_rebind_moved)."""
        if self._h is None:
            raise TamfError("the training step is closed")
        dev = self.device
        lab_np = check_labels(labels, self.input_dim)
        self._rebind_moved()
        (pr, sh, oe, ot), (B, T, F, nobj), num_np, side_d = encoder_batch(batch, obj_num, dev, self.input_dim, n_labels=lab_np.shape[0])
        clip_np = None
        if clip_ids is not None:
            clip_np = np.ascontiguousarray(torch.as_tensor(clip_ids).cpu().numpy() if isinstance(clip_ids, torch.Tensor) else clip_ids, dtype=np.int64)
            if clip_np.shape != (B,):
                raise ValueError(f"clip_ids must hold one id per clip: shape {clip_np.shape} for B = {B}")
        lab_d = torch.from_numpy(lab_np).to(dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        act = torch.empty(B, F, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _check(self._L.tamf_enctrain_step(
                self._h, B, T, nobj, num_np.ctypes.data_as(c_void_p) if num_np is not None else c_void_p(0), c_void_p(pr.data_ptr()),
                c_void_p(sh.data_ptr()), c_void_p(side_d.data_ptr()), c_void_p(oe.data_ptr()), c_void_p(ot.data_ptr()), c_void_p(lab_d.data_ptr()),
                clip_np.ctypes.data_as(c_void_p) if clip_np is not None else c_void_p(0), self.dropout, self.seed, int(step),
                c_void_p(loss.data_ptr()), c_void_p(act.data_ptr()), c_void_p(_stream_ptr(dev))))
        self._keep = [pr, sh, oe, ot, side_d, lab_d]
        acc = (act.argmax(1) == lab_d).float().mean()  # SegmentEncoderLoss's accuracy
        return {"loss": loss, "ce": loss, "acc": acc, "activation": act}
