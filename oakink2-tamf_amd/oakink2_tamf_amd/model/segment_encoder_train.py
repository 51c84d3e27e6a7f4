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
from ctypes import c_float, c_int32, c_uint32, c_uint64, c_void_p
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from ..hip_backend import _Arch, _stream_ptr, encoder_batch
from . import _train_step
from ._train_step import TrainStep, clip_id_vector

BUFFERS = ("classification_token", "hand_side_process.rh_embed", "hand_side_process.lh_embed", "sequence_pos_encoder.pe")
PREFIX = "tamf_enctrain_"


def lib() -> ctypes.CDLL:
    return _train_step.typed_lib(_lib.load_enctrain, PREFIX, {
        "step": [c_void_p, c_int32, c_int32, c_int32] + [c_void_p] * 8 + [c_float, c_uint64, c_uint32, c_void_p, c_void_p, c_void_p]})


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
    return _train_step.dropout_mask(lib(), PREFIX, seed, step, clip_id, site, rows, cols, p, device)


class SegmentEncoderTrainStep(TrainStep):
    """loss_and_grads(batch, labels) around a SegmentEncoder on a GPU.  Enables requires_grad on the trainable parameters (all of
    nn.Module.parameters(); the classification token, the hand-side embeddings and the PE table are buffers) and allocates their
    .grad.  dropout=None takes model.dropout."""

    LIB, PREFIX, BUFFERS = staticmethod(lib), PREFIX, BUFFERS

    def __init__(self, model, max_batch: int, max_frames: int, dropout: Optional[float] = None, seed: int = 0):
        self.input_dim = int(model.input_feats)
        a = model._arch
        arch = _Arch(a["input_dim"], a["obj_input_dim"], a["hand_shape_dim"], a["obj_embed_dim"], a["latent_dim"], a["ff_size"], a["num_layers"],
                     a["num_heads"], 0, 0, 2)
        super().__init__(model, arch, max_batch, max_frames, float(model.dropout if dropout is None else dropout), seed)

    def loss_and_grads(self, batch: Dict, labels, obj_num: Optional[Sequence[int]] = None, clip_ids: Optional[Sequence[int]] = None,
                       step: int = 0) -> Dict:
        """batch: "pose_repr" (B, T, input_dim), "hand_side" (B x "rh"/"lh"), "shape" (B, T, 10), "obj_embedding" (B, nobj, od),
        "obj_traj" (B, nobj, T, 9); labels (B,) integers in [0, input_dim) - the output head has input_dim logits.
        Fills p.grad of every trainable parameter (overwriting) -> {"loss", "ce", "acc", "activation"} (device tensors).
        optimizer.zero_grad() between steps is harmless and unnecessary: gradients set to None get their tensors back, and tensors
        that moved are bound again (_rebind_moved)."""
        self._require_open()
        dev = self.device
        lab_np = check_labels(labels, self.input_dim)
        self._rebind_moved()
        (pr, sh, oe, ot), (B, T, F, nobj), num_np, side_d = encoder_batch(batch, obj_num, dev, self.input_dim, n_labels=lab_np.shape[0])
        clip_np = clip_id_vector(clip_ids, B)
        lab_d = torch.from_numpy(lab_np).to(dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        act = torch.empty(B, F, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            self._call(
                "step", self._h, B, T, nobj, num_np.ctypes.data_as(c_void_p) if num_np is not None else c_void_p(0), c_void_p(pr.data_ptr()),
                c_void_p(sh.data_ptr()), c_void_p(side_d.data_ptr()), c_void_p(oe.data_ptr()), c_void_p(ot.data_ptr()), c_void_p(lab_d.data_ptr()),
                clip_np.ctypes.data_as(c_void_p) if clip_np is not None else c_void_p(0), self.dropout, self.seed, int(step),
                c_void_p(loss.data_ptr()), c_void_p(act.data_ptr()), c_void_p(_stream_ptr(dev)))
        self._keep = [pr, sh, oe, ot, side_d, lab_d]
        acc = (act.argmax(1) == lab_d).float().mean()  # SegmentEncoderLoss's accuracy
        return {"loss": loss, "ce": loss, "acc": acc, "activation": act}
