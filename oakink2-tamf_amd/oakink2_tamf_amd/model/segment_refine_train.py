"""SegmentRefineTrainStep - the training forward and backward of the refiner's trunk (SegmentRefineModel) on the gfx950 HIP library
libtamf_refinetrain.so (include/tamf_refinetrain.h).

forward() returns `refine_pose_repr` as a tensor that carries autograd: whatever loss the caller builds on it (the reference's goes
through MANO, nearest neighbours and float64 reductions), its .backward() reaches a torch.autograd.Function whose backward runs the HIP
backward of the trunk and fills the .grad of every parameter, OVERWRITING it.  The kernels read the parameters where torch keeps them,
so any torch.optim optimiser then steps on the device.  There is no PyTorch compute path and no fallback.  A forward serves one
backward; a second forward before the backward of the first is refused, like two backwards through one forward.

loss_and_grads() is the reference's whole step (train_refine.py:546-550) on this package's kernels.

After optimiser steps call model.refresh_hip_weights() before using the inference path (SegmentRefineModel.forward): the inference
context keeps its own composed copy of the weights.

Dropout masks are Philox draws keyed by (seed, step, clip id, site, element): see the header for the sites.  dropout_mask() returns the
keep-mask the step uses at one site.
"""
from __future__ import annotations

import ctypes
from ctypes import c_char_p, c_float, c_int32, c_int64, c_uint32, c_uint64, c_void_p
from typing import Dict, Mapping, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from ..hip_backend import _Arch, _dev_f32, _stream_ptr, hand_side_code, obj_num_vector
from . import _train_step
from ._train_step import TrainStep, clip_id_vector

BUFFERS = ("hand_side_process.rh_embed", "hand_side_process.lh_embed", "sequence_pos_encoder.pe")
PREFIX = "tamf_refinetrain_"


def lib() -> ctypes.CDLL:
    return _train_step.typed_lib(_lib.load_refinetrain, PREFIX, {
        "forward": [c_void_p, c_int32, c_int32, c_int32] + [c_void_p] * 8 + [c_float, c_uint64, c_uint32, c_void_p, c_void_p],
        "backward": [c_void_p, c_void_p, c_void_p], "set_profile": [c_void_p, c_int32], "get_profile": [c_void_p, c_char_p, c_int64]})


def dropout_mask(seed: int, step: int, clip_id: int, site: int, rows: int, cols: int, p: float, device=None) -> torch.Tensor:
    """the (rows, cols) bool keep-mask of one dropout site of one clip (tamf_refinetrain_dropout_mask)"""
    return _train_step.dropout_mask(lib(), PREFIX, seed, step, clip_id, site, rows, cols, p, device)


def check_refine_batch(batch: Mapping, h2o_dist, arch: Mapping[str, int], obj_num=None, clip_ids=None):
    """The Python-side refusals, device-free: -> (B, T, nobj, hand-side codes, int32 obj_num or None, int64 clip ids or None).
    ValueError for shapes that do not agree with each other or with the architecture, TypeError for a tensor that is not floating
    point."""
    x, sh, oe, ot = batch["sample_pose_repr"], batch["shape"], batch["obj_embedding"], batch["obj_traj"]
    for name, t in (("sample_pose_repr", x), ("shape", sh), ("obj_embedding", oe), ("obj_traj", ot), ("h2o_dist", h2o_dist)):
        if not torch.is_tensor(t) or not t.dtype.is_floating_point:
            raise TypeError(f"{name}: expected a floating-point tensor, got {t.dtype if torch.is_tensor(t) else type(t).__name__}")
    if x.dim() != 3 or x.shape[2] != arch["input_dim"]:
        raise ValueError(f"sample_pose_repr: expected (B, T, {arch['input_dim']}), got {tuple(x.shape)}")
    B, T, _ = (int(s) for s in x.shape)
    if B < 1 or T < 1:
        raise ValueError(f"sample_pose_repr: an empty batch {tuple(x.shape)}")
    if tuple(h2o_dist.shape) != (B, T, arch["h2o_dim"]):
        raise ValueError(f"h2o_dist: expected {(B, T, arch['h2o_dim'])}, got {tuple(h2o_dist.shape)}")
    if tuple(sh.shape) != (B, T, arch["hand_shape_dim"]):
        raise ValueError(f"shape: expected {(B, T, arch['hand_shape_dim'])}, got {tuple(sh.shape)}")
    if oe.dim() != 3 or oe.shape[0] != B or oe.shape[1] < 1 or oe.shape[2] != arch["obj_embed_dim"]:
        raise ValueError(f"obj_embedding: expected ({B}, nobj, {arch['obj_embed_dim']}), got {tuple(oe.shape)}")
    nobj = int(oe.shape[1])
    if tuple(ot.shape) != (B, nobj, T, arch["obj_input_dim"]):
        raise ValueError(f"obj_traj: expected {(B, nobj, T, arch['obj_input_dim'])}, got {tuple(ot.shape)}")
    side = [hand_side_code(hs) for hs in batch["hand_side"]]
    if len(side) != B:
        raise ValueError(f"hand_side: expected {B} entries, got {len(side)}")
    num_np = obj_num_vector(obj_num, B)
    if num_np is not None and (num_np.min() < 1 or num_np.max() > nobj):
        raise ValueError(f"obj_num must be in [1, nobj = {nobj}], got [{int(num_np.min())}, {int(num_np.max())}]")
    return B, T, nobj, side, num_np, clip_id_vector(clip_ids, B)


class PendingForward:
    """The claim of one forward on the step's workspace: taken by exactly one backward."""

    def __init__(self):
        self.open = True

    def take(self) -> None:
        if not self.open:
            raise RuntimeError("SegmentRefineTrainStep: this forward's activations are gone - a forward serves one backward (no second "
                               "backward, no retain_graph), and a later forward on the same step replaces them")
        self.open = False


class _TrunkFunction(torch.autograd.Function):
    """out = the forward's result, already computed; backward hands the incoming gradient to `backend.run_backward`, which writes the
    parameters' .grad itself.  `anchor` is a parameter: it makes the result part of the graph and receives no gradient from here."""

    @staticmethod
    def forward(ctx, backend, pending, out, anchor):
        ctx.backend, ctx.pending = backend, pending
        return out.view_as(out)

    @staticmethod
    def backward(ctx, grad):
        if torch.is_grad_enabled():  # (a backward that is itself recorded: create_graph=True)
            raise RuntimeError("SegmentRefineTrainStep: double backward is not supported (the HIP backward is first order only)")
        ctx.pending.take()
        ctx.backend.run_backward(grad)
        return None, None, None, None


class SegmentRefineTrainStep(TrainStep):
    """forward(batch) / loss_and_grads(batch, loss, obj_points) around a SegmentRefineModel on a GPU.  Enables requires_grad on the
    parameters (the hand-side embeddings and the PE table are buffers) and allocates their .grad.  dropout=None takes the model's
    (sequence_pos_encoder was built with it)."""

    LIB, PREFIX, BUFFERS = staticmethod(lib), PREFIX, BUFFERS

    def __init__(self, model, max_batch: int, max_frames: int, dropout: Optional[float] = None, seed: int = 0):
        dropout = float(model.seqTransEncoder.layers[0].dropout.p if dropout is None else dropout)
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout must be in [0, 1), got {dropout}")
        self.arch = dict(model._arch)
        a = self.arch
        arch = _Arch(a["input_dim"], a["obj_input_dim"], a["hand_shape_dim"], a["obj_embed_dim"], a["latent_dim"], a["ff_size"], a["num_layers"],
                     a["num_heads"], 0, a["h2o_dim"], 1)
        self._pending = None
        self._keep = None
        super().__init__(model, arch, max_batch, max_frames, dropout, seed)

    def dropout_mask(self, step: int, clip_id: int, site: int, rows: int, cols: int) -> torch.Tensor:
        """the keep-mask this step object uses (its seed and dropout) at one site of one clip"""
        return dropout_mask(self.seed, step, clip_id, site, rows, cols, self.dropout, self.device)

    def _sample_h2o_dist(self, batch: Mapping) -> torch.Tensor:
        """as SegmentRefineModel.forward: from the model's MANO layers, outside the graph"""
        m = self.model
        if m.mano_layer_rh is None and m.mano_layer_lh is None:
            raise KeyError("h2o_dist (B, T, 778) must be supplied - as the argument or as batch['h2o_dist'] - or the model built with "
                           "mano_layer_rh / mano_layer_lh")
        with torch.no_grad():
            hv, _, _ = m.batch_recover_mano_from_pose_repr(batch["sample_pose_repr"], batch["shape"], batch["hand_side"])
            return m.multi_object_h2o_dist(hv, batch["obj_list"], batch["obj_traj"], batch["obj_pointcloud"] if m.use_pc else batch["obj_verts"])

    def forward(self, batch: Mapping, h2o_dist: Optional[torch.Tensor] = None, obj_num: Optional[Sequence[int]] = None,
                clip_ids: Optional[Sequence[int]] = None, step: int = 0) -> torch.Tensor:
        """batch: "sample_pose_repr" (B, T, input_dim), "hand_side" (B x "rh"/"lh"), "shape" (B, T, 10), "obj_embedding" (B, nobj, od),
        "obj_traj" (B, nobj, T, 9); h2o_dist (B, T, 778) (else batch["h2o_dist"], else computed from the model's MANO layers without
        gradient).  obj_num: per-clip object counts (None: the mean over all nobj padded rows, the reference's forward); clip_ids: the
        keys of the dropout masks (None: the position in the batch).  -> refine_pose_repr (B, T, input_dim), carrying autograd to
        every parameter's .grad; sample_pose_repr is data and gets no gradient."""
        self._require_open()
        if self._pending is not None and self._pending.open:
            raise RuntimeError("SegmentRefineTrainStep: the previous forward has had no backward yet and a second forward would replace its "
                               "activations; run its backward first, or drop it with discard_forward()")
        if h2o_dist is None:
            h2o_dist = batch["h2o_dist"] if "h2o_dist" in batch else self._sample_h2o_dist(batch)
        B, T, nobj, side, num_np, clip_np = check_refine_batch(batch, h2o_dist, self.arch, obj_num, clip_ids)
        dev = self.device
        self._rebind_moved()
        x, hd = _dev_f32(batch["sample_pose_repr"], dev), _dev_f32(h2o_dist, dev)
        sh, oe, ot = _dev_f32(batch["shape"], dev), _dev_f32(batch["obj_embedding"], dev), _dev_f32(batch["obj_traj"], dev)
        side_d = torch.tensor(side, dtype=torch.uint8, device=dev)
        out = torch.empty(B, T, self.arch["input_dim"], dtype=torch.float32, device=dev)
        null = c_void_p(0)
        with torch.cuda.device(dev):
            self._call(
                "forward", self._h, B, T, nobj, num_np.ctypes.data_as(c_void_p) if num_np is not None else null, c_void_p(x.data_ptr()),
                c_void_p(hd.data_ptr()), c_void_p(sh.data_ptr()), c_void_p(side_d.data_ptr()), c_void_p(oe.data_ptr()), c_void_p(ot.data_ptr()),
                clip_np.ctypes.data_as(c_void_p) if clip_np is not None else null, self.dropout, self.seed, int(step),
                c_void_p(out.data_ptr()), c_void_p(_stream_ptr(dev)))
        self._keep = [x, hd, sh, oe, ot, side_d]  # (the backward reads sample_pose_repr and h2o_dist again)
        self._pending = PendingForward()
        anchor = next(self.model.parameters())
        return _TrunkFunction.apply(self, self._pending, out, anchor)

    def profile(self, on: bool) -> None:
        """measurement only: bracket every kernel launch of the following calls with events (tamf_refinetrain_set_profile)"""
        self._call("set_profile", self._h, int(bool(on)))

    def read_profile(self) -> Dict[str, tuple]:
        """{kind of kernel: (launches, milliseconds)} since the last read (tamf_refinetrain_get_profile); waits for the device"""
        buf = ctypes.create_string_buffer(1 << 16)
        self._call("get_profile", self._h, buf, len(buf))
        rows = [ln.split("\t") for ln in buf.value.decode().splitlines()]
        return {r[0]: (int(r[1]), float(r[2])) for r in rows}

    def discard_forward(self) -> None:
        """give up the pending forward (a forward whose loss is not going to be differentiated)"""
        if self._pending is not None:
            self._pending.open = False

    def run_backward(self, grad: torch.Tensor) -> None:
        """tamf_refinetrain_backward: the .grad of every parameter from d loss / d refine_pose_repr (called by autograd)"""
        self._require_open()
        g = _dev_f32(grad, self.device)
        self._rebind_moved()
        with torch.cuda.device(self.device):
            self._call("backward", self._h, c_void_p(g.data_ptr()), c_void_p(_stream_ptr(self.device)))
        self._keep = (self._keep or []) + [g]

    def loss_and_grads(self, batch: Mapping, loss, obj_points: torch.Tensor, obj_num: Optional[Sequence[int]] = None,
                       clip_ids: Optional[Sequence[int]] = None, step: int = 0, h2o_dist: Optional[torch.Tensor] = None) -> Dict:
        """The reference's step train_refine.py:546-550: trunk forward, decode_pose_repr, the differentiable MANO layers of `loss` (a
        HandInteractionLoss; one call per hand side), contact.merged_h2o_dist, the same for the ground truth batch["pose_repr"] without
        gradient, loss.refine_terms and .backward().  batch as forward() plus "pose_repr" (B, T, input_dim) and "mask" (B, T);
        obj_points (B, nobj, P, 3) in the object frame.  The sample's distance feature is h2o_dist, batch["h2o_dist"], or computed here
        the same way.  Afterwards every p.grad holds the gradient of the reference's loss.  -> the loss dict ("loss", "rec_joint",
        "rec_vert", "dist_h") with the reference's output keys (refine_*, target_*, sample_h2o_dist) under "output"."""
        dev = self.device
        on_dev = {k: (v if not torch.is_tensor(v) else _dev_f32(v, dev) if v.dtype.is_floating_point else v.to(dev)) for k, v in batch.items()}
        if h2o_dist is None:
            h2o_dist = on_dev.get("h2o_dist")
        try:
            total, terms, res = refine_step_loss(lambda h: self.forward(on_dev, h2o_dist=h, obj_num=obj_num, clip_ids=clip_ids, step=step),
                                                 on_dev, loss, _dev_f32(obj_points, dev), obj_num, h2o_dist)
            total.backward()
        finally:
            self.discard_forward()
        return {**{k: (v.detach() if torch.is_tensor(v) else v) for k, v in terms.items()}, "output": {k: v.detach() for k, v in res.items()}}


def recover_hands(layers: Mapping, pose_repr: torch.Tensor, shape: torch.Tensor, sides: Sequence[str]):
    """decode + MANO per hand side, as HandReconstructionLoss._per_side batches it: one layer call per side over all of its frames
    -> hand_verts (B, T, V, 3), hand_joints (B, T, 21, 3) with the wrist translation added, in the batch's order"""
    from .reconstruction_loss import decode_pose_repr

    B, T = pose_repr.shape[:2]
    verts, joints, order = [], [], []
    for side, layer in layers.items():
        rows = [i for i, s in enumerate(sides) if s == side]
        if not rows:
            continue
        idx = torch.as_tensor(rows, device=pose_repr.device)
        tsl, quat = decode_pose_repr(pose_repr[idx])
        out = layer(pose_coeffs=quat.reshape(len(rows) * T, -1, 4), betas=shape[idx].to(pose_repr.dtype).reshape(len(rows) * T, -1))
        verts.append(out.verts.reshape(len(rows), T, -1, 3).to(pose_repr.dtype) + tsl.unsqueeze(2))
        joints.append(out.joints.reshape(len(rows), T, -1, 3).to(pose_repr.dtype) + tsl.unsqueeze(2))
        order += rows
    if sorted(order) != list(range(B)):
        raise ValueError(f"unexpected hand_side: {list(sides)}")
    back = torch.as_tensor(np.argsort(np.asarray(order)), device=pose_repr.device)
    return torch.cat(verts, dim=0)[back], torch.cat(joints, dim=0)[back]


def refine_step_loss(trunk, batch: Mapping, loss, obj_points: torch.Tensor, obj_num=None, h2o_dist=None, merged_fn=None):
    """What surrounds the trunk in the reference's training step (model/segment_refine_model.py:192-248 and the loss), on tensors of
    one device and dtype: `trunk(sample_h2o_dist) -> refine_pose_repr` (B, T, input_dim) carrying autograd; `loss` a
    HandInteractionLoss whose `layers` are differentiable; merged_fn defaults to contact.merged_h2o_dist.
    -> (loss, loss dict, output dict with the reference's keys); the caller runs .backward()."""
    if merged_fn is None:
        from ..contact import merged_h2o_dist as merged_fn
    sides = list(batch["hand_side"])
    shape, traj = batch["shape"], batch["obj_traj"]
    res = {}
    with torch.no_grad():
        if h2o_dist is None:
            sv, sj = recover_hands(loss.layers, batch["sample_pose_repr"], shape, sides)
            h2o_dist = merged_fn(sv, traj, obj_points, obj_num)
            res["sample_hand_verts"], res["sample_hand_joints"] = sv, sj
        tv, tj = recover_hands(loss.layers, batch["pose_repr"], shape, sides)
        res["target_hand_verts"], res["target_hand_joints"] = tv, tj
        res["target_h2o_dist"] = merged_fn(tv, traj, obj_points, obj_num)
    res["sample_h2o_dist"] = h2o_dist
    out = trunk(h2o_dist)
    rv, rj = recover_hands(loss.layers, out, shape.to(out), sides)
    res["refine_pose_repr"], res["refine_hand_verts"], res["refine_hand_joints"] = out, rv, rj
    res["refine_h2o_dist"] = merged_fn(rv, traj.to(out), obj_points.to(out), obj_num)
    total, terms = loss.refine_terms(res, batch)
    return total, terms, res
