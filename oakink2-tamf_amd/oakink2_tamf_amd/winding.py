"""Generalized winding number of a triangle mesh: the HIP kernels of libtamf_winding.so (include/tamf_winding.h holds the definition).

    WindingSet(meshes)                          prepares a set of meshes once: validity mask, the valid faces in ascending order, upload
    WindingSet.points(points, mesh_id, ...)     many (mesh, rigid transform, slice of points) jobs -> w, inside
    WindingSet.lattice(m, ticks)                one mesh on an R^3 lattice -> w, inside
    winding_number(verts, faces, points)        the one-mesh convenience
    lattice_winding(verts, faces, ticks)        the same for a lattice

`inside` is |w| > 0.5: the sign for object meshes that are open or scanned, where the ray-parity test of geometry.mesh_contains /
voxelize_lattice (which presumes a closed mesh and is wrong where a vertical ray runs through mesh edges) gives whole columns the wrong
answer.  On a clean closed mesh the two agree.  The jobs are those of meshdist.MeshSet.distance, so a caller can take `dist` from
there and `inside` from here for the same points and transforms."""
from __future__ import annotations

from ctypes import c_char_p, c_int32, c_int64, c_uint32, c_void_p
from typing import Sequence

import numpy as np

from .meshdist import _mesh_arrays, valid_faces

CHUNK = 1024  # TAMF_WINDING_CHUNK
FOUR_PI = 12.566370614359172  # TAMF_WINDING_FOUR_PI
ROUTES = {None: 0, "auto": 0, "loop": 1, "spread": 2}  # the flags of tamf_winding_points
SIGNS = ("parity", "winding")  # what the consumers' `sign` option takes; "parity" is geometry.mesh_contains / voxelize_lattice


class WindingError(RuntimeError):
    pass


_lib = None


def _bind():
    global _lib
    if _lib is None:
        from . import _lib as L

        lib = L.load_winding()
        lib.tamf_winding_last_error.restype = c_char_p
        lib.tamf_winding_last_error.argtypes = []
        lib.tamf_winding_workspace.restype = c_int64
        lib.tamf_winding_workspace.argtypes = [c_int32, c_void_p, c_void_p, c_void_p]
        lib.tamf_winding_prepare.argtypes = [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]
        lib.tamf_winding_points_workspace.restype = c_int64
        lib.tamf_winding_points_workspace.argtypes = [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_uint32]
        lib.tamf_winding_points.argtypes = [c_void_p, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32,
                                            c_void_p, c_int64, c_void_p, c_void_p, c_void_p]
        lib.tamf_winding_lattice.argtypes = [c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]
        _lib = lib
    return _lib


def _check(rc: int) -> int:
    if rc < 0:
        raise WindingError(f"libtamf_winding: {_bind().tamf_winding_last_error().decode()} (status {rc})")
    return rc


def check_sign(sign: str) -> str:
    if sign not in SIGNS:
        raise ValueError(f"sign must be one of {SIGNS}, got {sign!r}")
    return sign


class WindingSet:
    """M triangle meshes [(verts (V, 3), faces (F, 3)), ...] packed once for the winding-number kernels.  Holds per mesh the validity
    mask (`valid`), the valid faces in ascending order (`valid_idx`), the offsets and the upload."""

    def __init__(self, meshes: Sequence, device=None, upload: bool = True):
        meshes = list(meshes)
        if not meshes:
            raise ValueError("WindingSet: no mesh")
        self.verts, self.faces, self.valid, self.valid_idx = [], [], [], []
        for m, (verts, faces) in enumerate(meshes):
            v, f = _mesh_arrays(verts, faces)
            ok = valid_faces(v, f)
            if not ok.any():
                raise WindingError(f"mesh {m} has no valid face (every face has a repeated index, one outside [0, {v.shape[0]}) or zero area)")
            self.verts.append(v)
            self.faces.append(f)
            self.valid.append(ok)
            self.valid_idx.append(np.flatnonzero(ok).astype(np.int32))
        self.M = len(meshes)
        off = lambda n: np.ascontiguousarray(np.concatenate([[0], np.cumsum(n)]).astype(np.int64))  # noqa: E731
        self.vert_off = off([v.shape[0] for v in self.verts])
        self.face_off = off([f.shape[0] for f in self.faces])
        self.valid_off = off([p.shape[0] for p in self.valid_idx])
        self.device = None
        self._ws = None
        if upload:
            self.upload(device)

    def upload(self, device=None) -> None:
        import torch

        from .hip_backend import _stream_ptr, require_gpu

        dev = require_gpu(device)
        lib = _bind()
        ptr = lambda a: a.ctypes.data_as(c_void_p)  # noqa: E731
        nbytes = _check(int(lib.tamf_winding_workspace(self.M, ptr(self.vert_off), ptr(self.face_off), ptr(self.valid_off))))
        v = np.ascontiguousarray(np.concatenate(self.verts))
        f = np.ascontiguousarray(np.concatenate(self.faces))
        p = np.ascontiguousarray(np.concatenate(self.valid_idx))
        with torch.cuda.device(dev):
            ws = torch.empty(nbytes // 8 + 2, dtype=torch.float64, device=dev)
            _check(lib.tamf_winding_prepare(ptr(v), ptr(f), self.M, ptr(self.vert_off), ptr(self.face_off), ptr(p), ptr(self.valid_off),
                                            ws.data_ptr(), nbytes, _stream_ptr(dev)))
        self.device, self._ws = dev, ws

    def points(self, points, mesh_id, transf=None, pt_off=None, pt_len=None, inside: bool = True, route=None):
        """points (P, 3) float32; job j takes points[pt_off[j] : pt_off[j] + pt_len[j]] through transf[j] ((J, 12) or (J, 3, 4) float64
        rows of [R | t]; None = identity) and takes the winding number of mesh mesh_id[j] there.  pt_off / pt_len None: every job takes
        all points.  -> w float64, inside bool or None: on the device, the jobs' outputs end to end in job order.  No host
        synchronisation.  `route`: None (the library decides from the call's sizes), "loop" or "spread" - the same bits either way."""
        import torch

        from .hip_backend import _stream_ptr

        if self._ws is None:
            raise WindingError("WindingSet.points: the set was not uploaded")
        if route not in ROUTES:
            raise ValueError(f"route must be one of {tuple(ROUTES)}, got {route!r}")
        dev = self.device
        p = torch.as_tensor(points)
        if p.dtype != torch.float32:
            raise ValueError(f"points must be float32 (the widening to float64 is then exact), got {p.dtype}")
        p = p.to(dev).contiguous().reshape(-1, 3)
        P = int(p.shape[0])
        mid = np.ascontiguousarray(np.asarray(mesh_id, dtype=np.int32).reshape(-1))
        J = int(mid.shape[0])
        off = np.zeros(J, np.int64) if pt_off is None else np.ascontiguousarray(np.asarray(pt_off, dtype=np.int64).reshape(-1))
        ln = np.full(J, P, np.int64) if pt_len is None else np.ascontiguousarray(np.asarray(pt_len, dtype=np.int64).reshape(-1))
        if transf is None:
            tr = np.ascontiguousarray(np.tile(np.eye(3, 4).reshape(1, 12), (J, 1)))
        else:
            tr = np.ascontiguousarray(np.asarray(transf, dtype=np.float64).reshape(J, 12) if J else np.zeros((0, 12)))
        if off.shape[0] != J or ln.shape[0] != J:
            raise ValueError("one offset, length, mesh id and transform per job")
        n_out = int(np.clip(ln, 0, None).sum())
        w = torch.empty(n_out, dtype=torch.float64, device=dev)
        ins = torch.empty(n_out, dtype=torch.uint8, device=dev) if inside else None
        if J == 0:
            return w, (ins.bool() if inside else None)
        lib = _bind()
        ptr = lambda a: a.ctypes.data_as(c_void_p)  # noqa: E731
        flags = ROUTES[route]
        jbytes = _check(int(lib.tamf_winding_points_workspace(J, self.M, ptr(mid), ptr(ln), ptr(self.valid_off), flags)))
        with torch.cuda.device(dev):
            jws = torch.empty(jbytes // 8 + 2, dtype=torch.float64, device=dev)
            _check(lib.tamf_winding_points(self._ws.data_ptr(), self.M, p.data_ptr() if P else None, P, J, ptr(mid), ptr(tr), ptr(off), ptr(ln),
                                           ptr(self.valid_off), flags, jws.data_ptr(), jbytes, w.data_ptr(), ins.data_ptr() if inside else None,
                                           _stream_ptr(dev)))
        return w, (ins.bool() if inside else None)

    def lattice(self, mesh: int, ticks, inside: bool = True):
        """ticks (R, 3) float64 -> (w float64 (R, R, R), inside bool (R, R, R) or None) on the device: element [i, j, k] is taken at
        (ticks[i,0], ticks[j,1], ticks[k,2])"""
        import torch

        from .hip_backend import _stream_ptr

        if self._ws is None:
            raise WindingError("WindingSet.lattice: the set was not uploaded")
        dev = self.device
        tk = torch.as_tensor(ticks).to(device=dev, dtype=torch.float64).contiguous()
        if tk.dim() != 2 or tk.shape[1] != 3:
            raise ValueError("ticks must be (R, 3)")
        R = int(tk.shape[0])
        w = torch.empty((max(R, 0),) * 3, dtype=torch.float64, device=dev)
        ins = torch.empty((max(R, 0),) * 3, dtype=torch.uint8, device=dev) if inside else None
        with torch.cuda.device(dev):
            _check(_bind().tamf_winding_lattice(self._ws.data_ptr(), self.M, int(mesh), tk.data_ptr(), R, w.data_ptr(),
                                                ins.data_ptr() if inside else None, _stream_ptr(dev)))
        return w, (ins.bool() if inside else None)


def winding_number(verts, faces, points, inside: bool = True, device=None):
    """points (P, 3) float32 against one mesh, as they are (identity pose) -> w (P,), inside (P,) or None"""
    return WindingSet([(verts, faces)], device=device).points(points, [0], inside=inside)


def lattice_winding(verts, faces, ticks, inside: bool = True, device=None):
    """-> (w float64 (R, R, R), inside bool (R, R, R) or None) of every lattice point (ticks[i,0], ticks[j,1], ticks[k,2])"""
    import torch

    if device is None and isinstance(ticks, torch.Tensor) and ticks.is_cuda:
        device = ticks.device
    return WindingSet([(verts, faces)], device=device).lattice(0, ticks, inside=inside)


__all__ = ["CHUNK", "FOUR_PI", "SIGNS", "WindingError", "WindingSet", "winding_number", "lattice_winding", "check_sign"]
