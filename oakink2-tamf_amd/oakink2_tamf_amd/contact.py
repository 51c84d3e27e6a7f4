"""The signed nearest-neighbour distances between hand vertices and object points that the training losses' `dist_h` / `dist_o` terms
are built on, with autograd for the hand vertices (libtamf_contact.so, include/tamf_contact.h).

signed_contact_distance  reference: point2point_signed (model/loss/chamfer_distance.py:4-64) as InteractionSegmentExtraLoss calls it
                         per clip and per object (model/interaction_segment_extra_loss.py:146-158), here for all clips, objects and
                         frames in one call.  The reference takes the indices from the external chamfer_distance CUDA package and
                         recomputes the differences itself; the kernels do both.
merged_h2o_dist          reference: SegmentRefineModel.multi_object_h2o_dist (model/segment_refine_model.py:142-168), with a gradient
                         (geometry.multi_object_h2o_dist is the inference version of the same quantity)

The gradient reaches `hand_verts` only.  The normals enter through a sign, which has a zero derivative, and the reference treats the
objects' trajectory and points as data.  First order only: a double backward raises.  No CPU or torch fall-back."""
from __future__ import annotations

import ctypes
from ctypes import c_int32, c_void_p
from typing import Optional, Sequence

import torch

_bound = None


def _bind():
    global _bound
    if _bound is None:
        from . import _lib

        lib = _lib.load_contact()
        lib.tamf_contact_last_error.restype = ctypes.c_char_p
        lib.tamf_contact_last_error.argtypes = []
        lib.tamf_contact_forward.argtypes = [c_void_p] * 5 + [c_int32] * 5 + [c_void_p] * 5
        lib.tamf_contact_backward.argtypes = [c_void_p] * 4 + [c_int32] * 5 + [c_void_p] * 7
        _bound = lib
    return _bound


def _check(lib, rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"libtamf_contact: {lib.tamf_contact_last_error().decode()} (status {rc})")


def _ptr(t):
    return None if t is None else t.data_ptr()


def check_shapes(hand_verts, hand_normals, obj_traj, obj_points, obj_num):
    """The Python-side refusals, device-free: -> (B, T, V, nobj, P, counts or None).  obj_num[b] outside [1, nobj] is refused here
    because the kernels cannot: they would treat a count above nobj as nobj and a count below 1 as a clip without objects."""
    if hand_verts.dim() != 4 or hand_verts.shape[3] != 3:
        raise ValueError(f"hand_verts: expected (B, T, V, 3), got {tuple(hand_verts.shape)}")
    B, T, V, _ = (int(s) for s in hand_verts.shape)
    if hand_normals is not None and tuple(hand_normals.shape) != (B, T, V, 3):
        raise ValueError(f"hand_normals: expected {(B, T, V, 3)} as hand_verts, got {tuple(hand_normals.shape)}")
    if obj_points.dim() != 4 or obj_points.shape[0] != B or obj_points.shape[3] != 3:
        raise ValueError(f"obj_points: expected ({B}, nobj, P, 3), got {tuple(obj_points.shape)}")
    nobj, P = int(obj_points.shape[1]), int(obj_points.shape[2])
    if tuple(obj_traj.shape) != (B, nobj, T, 9):
        raise ValueError(f"obj_traj: expected {(B, nobj, T, 9)}, got {tuple(obj_traj.shape)}")
    counts = None
    if obj_num is not None:
        counts = [int(n) for n in obj_num]
        if len(counts) != B:
            raise ValueError(f"obj_num: expected {B} counts, got {len(counts)}")
        for b, n in enumerate(counts):
            if not 1 <= n <= nobj:
                raise ValueError(f"obj_num[{b}] = {n} of clip {b} is outside [1, nobj = {nobj}]")
    return B, T, V, nobj, P, counts


def contact_forward_raw(hv, nrm, tr, pts, on, want_h2o: bool = True, want_o2h: bool = True):
    """tamf_contact_forward on float32 contiguous device tensors (on: int32 (B,) or None) -> (h2o, h2o_idx, o2h_signed, o2h_idx),
    a skipped direction's pair being None"""
    from .hip_backend import _stream_ptr

    dev = hv.device
    B, T, V, _ = hv.shape
    nobj, P = pts.shape[1], pts.shape[2]
    h2o = torch.empty((B, nobj, T, V), dtype=torch.float32, device=dev) if want_h2o else None
    h2o_idx = torch.empty((B, nobj, T, V), dtype=torch.int32, device=dev) if want_h2o else None
    o2h = torch.empty((B, nobj, T, P), dtype=torch.float32, device=dev) if want_o2h else None
    o2h_idx = torch.empty((B, nobj, T, P), dtype=torch.int32, device=dev) if want_o2h else None
    lib = _bind()
    with torch.cuda.device(dev):
        _check(lib, lib.tamf_contact_forward(_ptr(hv), _ptr(nrm), _ptr(tr), _ptr(pts), _ptr(on), B, T, V, nobj, P, _ptr(h2o), _ptr(h2o_idx),
                                             _ptr(o2h), _ptr(o2h_idx), _stream_ptr(dev)))
    return h2o, h2o_idx, o2h, o2h_idx


def contact_backward_raw(hv, tr, pts, on, h2o_idx, g_h2o, o2h_signed, o2h_idx, g_o2h):
    """tamf_contact_backward on float32 / int32 contiguous device tensors -> g_hand (B, T, V, 3); g_h2o or g_o2h may be None, not both"""
    from .hip_backend import _stream_ptr

    dev = hv.device
    B, T, V, _ = hv.shape
    nobj, P = pts.shape[1], pts.shape[2]
    g = torch.empty((B, T, V, 3), dtype=torch.float32, device=dev)
    lib = _bind()
    with torch.cuda.device(dev):
        _check(lib, lib.tamf_contact_backward(_ptr(hv), _ptr(tr), _ptr(pts), _ptr(on), B, T, V, nobj, P, _ptr(h2o_idx), _ptr(g_h2o),
                                              _ptr(o2h_signed), _ptr(o2h_idx), _ptr(g_o2h), _ptr(g), _stream_ptr(dev)))
    return g


class _ContactFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hv, nrm, tr, pts, on, want_o2h):
        h2o, h2o_idx, o2h, o2h_idx = contact_forward_raw(hv, nrm, tr, pts, on, True, want_o2h)
        ctx.save_for_backward(hv, tr, pts, on, h2o_idx, o2h, o2h_idx)
        ctx.set_materialize_grads(False)  # an output nothing depends on arrives as None and is passed as NULL
        if not want_o2h:
            return h2o
        ctx.mark_non_differentiable(o2h_idx)
        return o2h, h2o, o2h_idx

    @staticmethod
    def backward(ctx, *grads):
        if torch.is_grad_enabled():  # (a backward that is itself recorded: create_graph=True)
            raise RuntimeError("signed_contact_distance: double backward is not supported (the HIP backward is first order only; "
                               "call backward / autograd.grad without create_graph)")
        hv, tr, pts, on, h2o_idx, o2h, o2h_idx = ctx.saved_tensors
        g_o2h, g_h2o = (grads[0], grads[1]) if len(grads) == 3 else (None, grads[0])
        if (g_o2h is None and g_h2o is None) or not ctx.needs_input_grad[0]:
            return (None,) * 6
        f32 = lambda g: None if g is None else g.to(torch.float32).contiguous()  # noqa: E731
        g = contact_backward_raw(hv, tr, pts, on, h2o_idx, f32(g_h2o), o2h, o2h_idx, f32(g_o2h))
        return g, None, None, None, None, None


def signed_contact_distance(hand_verts: torch.Tensor, hand_normals: Optional[torch.Tensor], obj_traj: torch.Tensor, obj_points: torch.Tensor,
                            obj_num: Optional[Sequence[int]] = None, want_o2h: bool = True):
    """hand_verts (B,T,V,3), hand_normals (B,T,V,3) or None, obj_traj (B,nobj,T,9) = tsl | rot6d, obj_points (B,nobj,P,3) in the object
    frame, obj_num per clip -> (o2h_signed (B,nobj,T,P), h2o (B,nobj,T,V), o2h_idx (B,nobj,T,P) int32), PER OBJECT: point2point_signed's
    triple for every clip, object and frame.  o2h_signed is the distance of an object point to its nearest hand vertex, negative
    where the point lies behind that vertex's normal (unsigned without normals); h2o the distance of a hand vertex to the object's
    nearest point.  Rows of padded objects (o >= obj_num[b]) are 0, with index -1.  `want_o2h=False` computes h2o only and returns
    (None, h2o, None).  Autograd reaches hand_verts only."""
    from .hip_backend import _dev_f32, require_gpu

    B, T, V, nobj, P, counts = check_shapes(hand_verts, hand_normals, obj_traj, obj_points, obj_num)
    dev = require_gpu(hand_verts.device)
    hv = hand_verts.to(device=dev, dtype=torch.float32).contiguous()  # (stays in the graph)
    nrm = None if hand_normals is None or not want_o2h else _dev_f32(hand_normals, dev)
    tr, pts = _dev_f32(obj_traj, dev), _dev_f32(obj_points, dev)
    on = None if counts is None else torch.as_tensor(counts, dtype=torch.int32, device=dev)
    if torch.is_grad_enabled() and hv.requires_grad:
        out = _ContactFunction.apply(hv, nrm, tr, pts, on, bool(want_o2h))
        return out if want_o2h else (None, out, None)
    h2o, _, o2h, o2h_idx = contact_forward_raw(hv.detach(), nrm, tr, pts, on, True, bool(want_o2h))
    return o2h, h2o, o2h_idx


def merged_h2o_dist(hand_verts: torch.Tensor, obj_traj: torch.Tensor, obj_points: torch.Tensor, obj_num: Optional[Sequence[int]] = None,
                    contact_fn=None) -> torch.Tensor:
    """-> (B,T,V): the distance of every hand vertex to the nearest point of any real object of its clip, the refiner's feature and
    the `refine_h2o_dist` of its loss - geometry.multi_object_h2o_dist bit for bit, with a gradient for hand_verts.  The minimum over
    the objects is a torch `min`, so autograd carries it (to the first of equal objects)."""
    fn = signed_contact_distance if contact_fn is None else contact_fn
    _, h2o, _ = fn(hand_verts, None, obj_traj, obj_points, obj_num, want_o2h=False)
    if obj_num is not None:
        nobj = h2o.shape[1]
        real = torch.arange(nobj, device=h2o.device)[None, :] < torch.as_tensor([int(n) for n in obj_num], device=h2o.device)[:, None]
        h2o = torch.where(real[:, :, None, None], h2o, torch.full_like(h2o, float("inf")))
    return h2o.min(dim=1).values


__all__ = ["signed_contact_distance", "merged_h2o_dist", "contact_forward_raw", "contact_backward_raw", "check_shapes"]
