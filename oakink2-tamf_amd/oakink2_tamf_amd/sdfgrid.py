"""How deep hand vertices lie inside objects, read from the objects' precomputed signed distance lattices by a trilinear lookup, with
autograd for the hand vertices (libtamf_sdfgrid.so, include/tamf_sdfgrid.h: the definition, operation by operation).  It is what the
`pen` term of model/interaction_loss.HandInteractionLoss is built on.  The term is this package's own: the reference trains without it.

pack_grid            one SDFData field dict (meshdist.process_sdf's, or a pickle script/process_object_sdf.sh wrote) -> the lattice the
                     kernels read: values (R^3,) float32, res, origin, step.  Device-free.
SdfGridSet           G packed lattices end to end in device memory
penetration_depth    hand_verts, obj_traj, grid_id -> depth (B, nobj, T, V), positive inside (the sign of the file: that of
                     check_mesh_contains for process_sdf's files, as for the SIV and PD scores), 0 outside the object or its lattice.
                     Its resolution is the lattice's: between lattice points the depth is interpolated.
grid_ids             the (B, max nobj) int32 table of a batch from the items' obj_list

The gradient reaches `hand_verts` only: the trajectory and the lattice are data.  First order only: a double backward raises.  No CPU
or torch fall-back."""
from __future__ import annotations

import ctypes
import os
import pickle
from ctypes import c_int32, c_void_p
from typing import Dict, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

MIN_RES, MAX_RES = 2, 512  # TAMF_SDFGRID_MIN_RES / _MAX_RES
POINT_RTOL = 1e-6  # of the extent: how far `point`'s ends may lie from origin and origin + (R - 1) step (a millionth of the box)

_bound = None


def _bind():
    global _bound
    if _bound is None:
        from . import _lib

        lib = _lib.load_sdfgrid()
        lib.tamf_sdfgrid_last_error.restype = ctypes.c_char_p
        lib.tamf_sdfgrid_last_error.argtypes = []
        lib.tamf_sdfgrid_forward.argtypes = [c_void_p] * 5 + [c_int32] + [c_void_p] * 4 + [c_int32] * 4 + [c_void_p] * 3
        lib.tamf_sdfgrid_backward.argtypes = [c_void_p] * 5 + [c_int32] + [c_void_p] * 4 + [c_int32] * 4 + [c_void_p] * 3
        _bound = lib
    return _bound


def _check(lib, rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"libtamf_sdfgrid: {lib.tamf_sdfgrid_last_error().decode()} (status {rc})")


def _ptr(t):
    return None if t is None else t.data_ptr()


def pack_grid(fields: Mapping) -> Dict:
    """SDFData fields -> {"values" (R^3,) float32, "res" R, "origin" (3,) float64, "step" (3,) float64}.
    origin = mesh_center - extent_expanded / 2 and step = extent_expanded / (R - 1): the spacing of the file's linspace (NOT its
    tick_unit, which is extent_expanded / R).  The lattice's object-frame position is the file's `point` field - the centred tick plus
    mesh_center, once - and its two ends are checked against origin and origin + (R - 1) step.  ValueError: a resolution outside
    [2, 512], an `sdf` whose length is not R^3, an extent that is not positive and finite, a `point` field that disagrees."""
    for key in ("resolution", "mesh_center", "extent_expanded", "point", "sdf"):
        if key not in fields:
            raise ValueError(f"SDF fields lack {key!r}")
    res = int(fields["resolution"])
    if not MIN_RES <= res <= MAX_RES:
        raise ValueError(f"resolution {res} outside [{MIN_RES}, {MAX_RES}]")
    sdf = np.asarray(fields["sdf"]).reshape(-1)
    if sdf.shape[0] != res ** 3:
        raise ValueError(f"sdf holds {sdf.shape[0]} values, resolution {res} needs {res ** 3}")
    center = np.asarray(fields["mesh_center"], dtype=np.float64).reshape(-1)
    ext = np.asarray(fields["extent_expanded"], dtype=np.float64).reshape(-1)
    if center.shape != (3,) or ext.shape != (3,):
        raise ValueError("mesh_center and extent_expanded must hold 3 numbers each")
    if not (np.isfinite(ext).all() and (ext > 0).all() and np.isfinite(center).all()):
        raise ValueError(f"extent_expanded {ext.tolist()} is not positive and finite on every axis (a flat mesh has no lattice)")
    origin = center - ext / 2.0
    step = ext / float(res - 1)
    point = np.asarray(fields["point"], dtype=np.float64)
    if point.shape != (res ** 3, 3):
        raise ValueError(f"point has shape {point.shape}, resolution {res} needs {(res ** 3, 3)}")
    last = origin + float(res - 1) * step
    tol = POINT_RTOL * ext
    if not ((np.abs(point[0] - origin) <= tol).all() and (np.abs(point[-1] - last) <= tol).all()):
        raise ValueError(f"the point field runs from {point[0].tolist()} to {point[-1].tolist()}, but mesh_center and extent_expanded put the "
                         f"lattice from {origin.tolist()} to {last.tolist()}")
    return {"values": np.ascontiguousarray(sdf, dtype=np.float32), "res": res, "origin": origin, "step": step}


class SdfGridSet:
    """`grids`: a sequence of SDFData field dicts, packed by pack_grid (a dict pack_grid returned is taken as it is).  The host arrays (`values`, `grid_off`, `res`, `origin`,
    `step`, `packed`) are always there; with `upload` the set also lives on `device` (None: the current one), which is what
    penetration_depth reads.  upload=False touches no GPU."""

    def __init__(self, grids: Sequence[Mapping], device=None, upload: bool = True):
        self.packed = [g if "values" in g and "res" in g else pack_grid(g) for g in grids]
        if not self.packed:
            raise ValueError("SdfGridSet: no grids")
        self.G = len(self.packed)
        self.res = np.asarray([p["res"] for p in self.packed], dtype=np.int32)
        self.grid_off = np.concatenate([[0], np.cumsum([int(r) ** 3 for r in self.res])]).astype(np.int64)
        self.values = np.concatenate([p["values"] for p in self.packed]).astype(np.float32)
        self.origin = np.ascontiguousarray(np.stack([p["origin"] for p in self.packed]), dtype=np.float64)
        self.step = np.ascontiguousarray(np.stack([p["step"] for p in self.packed]), dtype=np.float64)
        self.index_of: Dict[str, int] = {}  # obj_id -> index in the set (from_prefix fills it)
        self.device = None
        self._dev = None
        if upload:
            self.upload(device)

    def upload(self, device=None) -> "SdfGridSet":
        """copies the packed set to `device` (None: the current one); -> self"""
        from .hip_backend import require_gpu

        self.device = require_gpu(device)
        self._dev = tuple(torch.from_numpy(a).to(self.device) for a in (self.values, self.grid_off, self.res, self.origin, self.step))
        return self

    @classmethod
    def from_prefix(cls, prefix: str, obj_ids: Sequence[str], device=None, upload: bool = True) -> Tuple[Optional["SdfGridSet"], list]:
        """`prefix/<obj_id>.pkl` per id, in the order given -> (the set, or None when no id has a file; the ids that had no file).
        The set's `index_of` maps an id to its index in the set."""
        fields, index_of, missing = [], {}, []
        for oid in obj_ids:
            path = os.path.join(prefix, f"{oid}.pkl")
            if not os.path.exists(path):
                missing.append(oid)
                continue
            with open(path, "rb") as f:
                d = pickle.load(f)
            try:
                packed = pack_grid(d)  # (the file's `point` field, 24 R^3 bytes, is dropped here)
            except ValueError as e:
                raise ValueError(f"{path}: {e}") from None
            index_of[oid] = len(fields)
            fields.append(packed)
        if not fields:
            return None, missing
        out = cls(fields, device=device, upload=upload)
        out.index_of = index_of
        return out, missing

    def tensors(self):
        if self._dev is None:
            raise RuntimeError("SdfGridSet: the set was not uploaded")
        return self._dev

    def check_ids(self, grid_id) -> None:
        """ValueError unless every id lies in [-1, G): the kernels cannot report it (they would treat such an object as one without a lattice)"""
        g = torch.as_tensor(grid_id)
        if g.numel() and bool(((g < -1) | (g >= self.G)).any()):
            raise ValueError(f"grid_id outside [-1, G = {self.G}): [{int(g.min())}, {int(g.max())}]")

    def penetration_depth(self, hand_verts, obj_traj, grid_id, obj_num=None):
        return penetration_depth(self, hand_verts, obj_traj, grid_id, obj_num)


def check_shapes(hand_verts, obj_traj, grid_id, obj_num):
    """The Python-side refusals, device-free: -> (B, T, V, nobj, counts or None)"""
    if hand_verts.dim() != 4 or hand_verts.shape[3] != 3:
        raise ValueError(f"hand_verts: expected (B, T, V, 3), got {tuple(hand_verts.shape)}")
    B, T, V, _ = (int(s) for s in hand_verts.shape)
    if obj_traj.dim() != 4 or obj_traj.shape[0] != B or obj_traj.shape[2] != T or obj_traj.shape[3] != 9:
        raise ValueError(f"obj_traj: expected ({B}, nobj, {T}, 9), got {tuple(obj_traj.shape)}")
    nobj = int(obj_traj.shape[1])
    if tuple(grid_id.shape) != (B, nobj):
        raise ValueError(f"grid_id: expected {(B, nobj)}, got {tuple(grid_id.shape)}")
    counts = None
    if obj_num is not None:
        counts = [int(n) for n in obj_num]
        if len(counts) != B:
            raise ValueError(f"obj_num: expected {B} counts, got {len(counts)}")
        for b, n in enumerate(counts):
            if not 1 <= n <= nobj:
                raise ValueError(f"obj_num[{b}] = {n} of clip {b} is outside [1, nobj = {nobj}]")
    return B, T, V, nobj, counts


def sdfgrid_forward_raw(grids: SdfGridSet, hv, tr, gid, on, want_cell: bool = False):
    """tamf_sdfgrid_forward on float32 / int32 contiguous device tensors (on: int32 (B,) or None) -> (depth, cell or None)"""
    from .hip_backend import _stream_ptr

    dev = hv.device
    B, T, V, _ = hv.shape
    nobj = tr.shape[1]
    depth = torch.empty((B, nobj, T, V), dtype=torch.float32, device=dev)
    cell = torch.empty((B, nobj, T, V), dtype=torch.int32, device=dev) if want_cell else None
    lib = _bind()
    with torch.cuda.device(dev):
        _check(lib, lib.tamf_sdfgrid_forward(*(_ptr(t) for t in grids.tensors()), grids.G, _ptr(hv), _ptr(tr), _ptr(gid), _ptr(on), B, T, V, nobj,
                                             _ptr(depth), _ptr(cell), _stream_ptr(dev)))
    return depth, cell


def sdfgrid_backward_raw(grids: SdfGridSet, hv, tr, gid, on, g_depth):
    """tamf_sdfgrid_backward on float32 / int32 contiguous device tensors -> g_hand (B, T, V, 3)"""
    from .hip_backend import _stream_ptr

    dev = hv.device
    B, T, V, _ = hv.shape
    nobj = tr.shape[1]
    g = torch.empty((B, T, V, 3), dtype=torch.float32, device=dev)
    lib = _bind()
    with torch.cuda.device(dev):
        _check(lib, lib.tamf_sdfgrid_backward(*(_ptr(t) for t in grids.tensors()), grids.G, _ptr(hv), _ptr(tr), _ptr(gid), _ptr(on), B, T, V, nobj,
                                              _ptr(g_depth), _ptr(g), _stream_ptr(dev)))
    return g


class _SdfGridFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hv, tr, gid, on, grids):
        depth, _ = sdfgrid_forward_raw(grids, hv, tr, gid, on)
        ctx.save_for_backward(hv, tr, gid, on)
        ctx.grids = grids
        return depth

    @staticmethod
    def backward(ctx, g_depth):
        if torch.is_grad_enabled():  # (a backward that is itself recorded: create_graph=True)
            raise RuntimeError("penetration_depth: double backward is not supported (the HIP backward is first order only; "
                               "call backward / autograd.grad without create_graph)")
        hv, tr, gid, on = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        g = sdfgrid_backward_raw(ctx.grids, hv, tr, gid, on, g_depth.to(torch.float32).contiguous())
        return g, None, None, None, None


def penetration_depth(grids: SdfGridSet, hand_verts, obj_traj, grid_id, obj_num: Optional[Sequence[int]] = None):
    """hand_verts (B,T,V,3), obj_traj (B,nobj,T,9) = tsl | rot6d, grid_id (B,nobj) integers in [-1, G) (-1: the object has no lattice),
    obj_num per clip -> depth (B,nobj,T,V) float32: how deep every vertex lies inside every object, 0 outside the object, outside its
    lattice, for a padded object (o >= obj_num[b]) and for one without a lattice.  Autograd reaches hand_verts only."""
    from .hip_backend import _dev_f32, require_gpu

    gid = torch.as_tensor(grid_id)
    B, T, V, nobj, counts = check_shapes(hand_verts, obj_traj, gid, obj_num)
    dev = require_gpu(hand_verts.device)
    if grids.device != dev:
        raise ValueError(f"the grid set lives on {grids.device}, hand_verts on {dev}")
    grids.check_ids(gid)
    hv = hand_verts.to(device=dev, dtype=torch.float32).contiguous()  # (stays in the graph)
    tr = _dev_f32(obj_traj, dev)
    gid = gid.detach().to(device=dev, dtype=torch.int32).contiguous()
    on = None if counts is None else torch.as_tensor(counts, dtype=torch.int32, device=dev)
    if torch.is_grad_enabled() and hv.requires_grad:
        return _SdfGridFunction.apply(hv, tr, gid, on, grids)
    return sdfgrid_forward_raw(grids, hv.detach(), tr, gid, on)[0]


def grid_ids(obj_lists: Sequence[Sequence[str]], index_of: Mapping[str, int]):
    """The items' obj_list -> the (B, max nobj) int32 table: index_of[obj_id], -1 for an object without a lattice and for padding"""
    nobj = max((len(ol) for ol in obj_lists), default=0)
    if nobj < 1:
        raise ValueError("grid_ids: no objects")
    out = np.full((len(obj_lists), nobj), -1, np.int32)
    for b, ol in enumerate(obj_lists):
        for o, oid in enumerate(ol):
            out[b, o] = int(index_of.get(oid, -1))
    return torch.from_numpy(out)


__all__ = ["SdfGridSet", "pack_grid", "penetration_depth", "grid_ids", "sdfgrid_forward_raw", "sdfgrid_backward_raw", "check_shapes", "MIN_RES", "MAX_RES"]
