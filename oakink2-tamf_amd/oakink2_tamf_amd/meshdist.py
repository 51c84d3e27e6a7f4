"""Exact point-to-mesh distance: the bit-defined HIP kernels of libtamf_meshdist.so (include/tamf_meshdist.h holds the definition).

    MeshSet(meshes)                           prepares a set of meshes once: validity mask, Morton permutation, inside-test rescaling, upload
    MeshSet.distance(points, mesh_id, ...)    many (mesh, rigid transform, slice of points) jobs in one launch -> dist, face, inside
    MeshSet.lattice(m, ticks)                 one mesh on an R^3 lattice
    mesh_distance(verts, faces, points)       the one-mesh convenience
    lattice_distance(verts, faces, ticks)     the same for a lattice
    process_sdf(verts, faces, ...)            the reference's SDFData fields (dev_fn/util/sdf_util.py:59-99), all twelve, without pysdf

The distance is unsigned and exact to the stated definition; the sign, where one is given (`inside`, process_sdf's `sdf`), is that of
the reference's check_mesh_contains (geometry.mesh_contains / voxelize_lattice), which presumes a closed mesh - not pysdf's.
process_sdf(sign="winding") takes the sign from the generalized winding number instead (winding.py), for meshes that are not closed."""
from __future__ import annotations

from ctypes import c_char_p, c_int32, c_int64, c_uint32, c_void_p
from typing import Dict, Sequence, Tuple

import numpy as np

TILE = 64  # TAMF_MESHDIST_TILE
MORTON_BITS = 10  # per axis
HASH_RESOLUTION = 512  # geometry.mesh_contains' default
SDF_FIELDS = ("mesh_center", "bbox", "bbox_centered", "bbox_centered_expanded", "bbox_expanded", "bbox_expand_ratio", "resolution", "extent",
              "extent_expanded", "tick_unit", "point", "sdf")  # SDFData (sdf_util.py:40-56)


class MeshDistError(RuntimeError):
    pass


_lib = None


def _bind():
    global _lib
    if _lib is None:
        from . import _lib as L

        lib = L.load_meshdist()
        lib.tamf_meshdist_last_error.restype = c_char_p
        lib.tamf_meshdist_last_error.argtypes = []
        lib.tamf_meshdist_workspace.restype = c_int64
        lib.tamf_meshdist_workspace.argtypes = [c_int32, c_void_p, c_void_p, c_void_p]
        lib.tamf_meshdist_prepare.argtypes = [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                              c_void_p, c_int64, c_void_p]
        lib.tamf_meshdist_points_workspace.restype = c_int64
        lib.tamf_meshdist_points_workspace.argtypes = [c_int32]
        lib.tamf_meshdist_points.argtypes = [c_void_p, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32,
                                             c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]
        lib.tamf_meshdist_lattice.argtypes = [c_void_p, c_int32, c_int32, c_void_p, c_int32, c_uint32, c_void_p, c_void_p]
        _lib = lib
    return _lib


def _check(rc: int) -> int:
    if rc < 0:
        raise MeshDistError(f"libtamf_meshdist: {_bind().tamf_meshdist_last_error().decode()} (status {rc})")
    return rc


# ---------------------------------------------------------------------------------------------------------------------------------
# host side: which faces count, in what order they are packed
# ---------------------------------------------------------------------------------------------------------------------------------
def _mesh_arrays(verts, faces) -> Tuple[np.ndarray, np.ndarray]:
    import torch

    v = verts.detach().cpu().numpy() if isinstance(verts, torch.Tensor) else np.asarray(verts)
    f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1:
        raise ValueError(f"verts: expected (V, 3) with V >= 1, got {v.shape}")
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or f.dtype.kind not in "iu":
        raise ValueError(f"faces: expected integers of shape (F, 3) with F >= 1, got {f.dtype} {f.shape}")
    if f.size and (int(f.max()) > 2 ** 31 - 1 or int(f.min()) < -2 ** 31):
        raise ValueError("faces: an index does not fit int32")
    return np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int32)


def in_range_faces(verts, faces) -> np.ndarray:
    """bool (F,): every index in [0, V) - the faces that can be read at all (the inside test's mesh)"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < np.asarray(verts).reshape(-1, 3).shape[0])).all(1)


def valid_faces(verts, faces) -> np.ndarray:
    """bool (F,): indices in [0, V), pairwise different, area > 0 by mesh_io.face_areas - mesh_report's and the surface sampler's predicate"""
    from .mesh_io import face_areas

    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = in_range_faces(v, f) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    area = np.zeros(f.shape[0])
    area[ok] = face_areas(v, f[ok])
    return ok & (area > 0)


def _spread3(x: np.ndarray) -> np.ndarray:
    """the low 10 bits of x, two zero bits between neighbours"""
    x = x.astype(np.uint64) & np.uint64(0x3FF)
    x = (x | (x << np.uint64(16))) & np.uint64(0x030000FF)
    x = (x | (x << np.uint64(8))) & np.uint64(0x0300F00F)
    x = (x | (x << np.uint64(4))) & np.uint64(0x030C30C3)
    x = (x | (x << np.uint64(2))) & np.uint64(0x09249249)
    return x


def morton_codes(centroids) -> np.ndarray:
    """uint64 (n,): the 30-bit Morton code of each point on the 1024^3 grid over the points' bounding box (x the highest bit of a triple)"""
    c = np.asarray(centroids, dtype=np.float64).reshape(-1, 3)
    if c.shape[0] == 0:
        return np.zeros(0, np.uint64)
    lo, hi = c.min(0), c.max(0)
    span = np.where(hi > lo, hi - lo, 1.0)
    with np.errstate(invalid="ignore"):
        cell = np.floor((c - lo) / span * (2 ** MORTON_BITS - 1))
    cell = np.nan_to_num(cell, nan=0.0, posinf=2 ** MORTON_BITS - 1, neginf=0.0).clip(0, 2 ** MORTON_BITS - 1).astype(np.int64)
    return (_spread3(cell[:, 0]) << np.uint64(2)) | (_spread3(cell[:, 1]) << np.uint64(1)) | _spread3(cell[:, 2])


def morton_permutation(verts, faces, valid=None) -> np.ndarray:
    """int32 (n_valid,): the valid faces in Morton order of their centroids ((a + b) + c) / 3, equal codes by ascending index.  The
    order decides only how compact a tile is: the distance does not depend on it."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    idx = np.flatnonzero(valid_faces(v, f) if valid is None else np.asarray(valid, dtype=bool))
    tri = v[f[idx]]
    code = morton_codes(((tri[:, 0] + tri[:, 1]) + tri[:, 2]) / 3.0)
    return idx[np.argsort(code, kind="stable")].astype(np.int32)


def contains_rescaling(verts, faces, resolution: int = HASH_RESOLUTION) -> Tuple[np.ndarray, np.ndarray]:
    """scale3, translate3 of the inside test as geometry.mesh_contains computes them (inside_mesh.py:21-26), over the faces given"""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    tri = v[np.asarray(faces, dtype=np.int64).reshape(-1, 3)].reshape(-1, 3)
    bmin, bmax = tri.min(axis=0), tri.max(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.ascontiguousarray((resolution - 1) / (bmax - bmin), dtype=np.float64)
        translate = np.ascontiguousarray(0.5 - scale * bmin, dtype=np.float64)
    return scale, translate


# ---------------------------------------------------------------------------------------------------------------------------------
# the prepared set
# ---------------------------------------------------------------------------------------------------------------------------------
class MeshSet:
    """M triangle meshes [(verts (V, 3), faces (F, 3)), ...] packed once for the distance kernels.  Holds per mesh the validity mask
    (`valid`), the Morton permutation (`perm`), scale3 / translate3 of the inside test (`scale3`, `translate3`), and the upload."""

    def __init__(self, meshes: Sequence, device=None, resolution: int = HASH_RESOLUTION, upload: bool = True):
        meshes = list(meshes)
        if not meshes:
            raise ValueError("MeshSet: no mesh")
        self.resolution = int(resolution)
        self.verts, self.faces, self.valid, self.perm = [], [], [], []
        sc, tr = [], []
        for m, (verts, faces) in enumerate(meshes):
            v, f = _mesh_arrays(verts, faces)
            ok = valid_faces(v, f)
            if not ok.any():
                raise MeshDistError(f"mesh {m} has no valid face (every face has a repeated index, one outside [0, {v.shape[0]}) or zero area)")
            s, t = contains_rescaling(v, f[in_range_faces(v, f)], self.resolution)
            self.verts.append(v)
            self.faces.append(f)
            self.valid.append(ok)
            self.perm.append(morton_permutation(v, f, ok))
            sc.append(s)
            tr.append(t)
        self.M = len(meshes)
        self.scale3, self.translate3 = np.ascontiguousarray(np.stack(sc)), np.ascontiguousarray(np.stack(tr))
        off = lambda n: np.ascontiguousarray(np.concatenate([[0], np.cumsum(n)]).astype(np.int64))  # noqa: E731
        self.vert_off = off([v.shape[0] for v in self.verts])
        self.face_off = off([f.shape[0] for f in self.faces])
        self.perm_off = off([p.shape[0] for p in self.perm])
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
        nbytes = _check(int(lib.tamf_meshdist_workspace(self.M, ptr(self.vert_off), ptr(self.face_off), ptr(self.perm_off))))
        v = np.ascontiguousarray(np.concatenate(self.verts))
        f = np.ascontiguousarray(np.concatenate(self.faces))
        p = np.ascontiguousarray(np.concatenate(self.perm))
        with torch.cuda.device(dev):
            ws = torch.empty(nbytes // 8 + 2, dtype=torch.float64, device=dev)
            _check(lib.tamf_meshdist_prepare(ptr(v), ptr(f), self.M, ptr(self.vert_off), ptr(self.face_off), ptr(p), ptr(self.perm_off),
                                             ptr(self.scale3), ptr(self.translate3), self.resolution, ws.data_ptr(), nbytes, _stream_ptr(dev)))
        self.device, self._ws = dev, ws

    def distance(self, points, mesh_id, transf=None, pt_off=None, pt_len=None, inside: bool = True, cull: bool = True):
        """points (P, 3) float32; job j takes points[pt_off[j] : pt_off[j] + pt_len[j]] through transf[j] ((J, 12) or (J, 3, 4) float64
        rows of [R | t]; None = identity) and measures them against mesh mesh_id[j].  pt_off / pt_len None: every job takes all points.
        -> dist float64, face int32 (the original index, local to the mesh), inside bool or None: on the device, the jobs' outputs end
        to end in job order.  One launch, no host synchronisation."""
        import torch

        from .hip_backend import _stream_ptr

        if self._ws is None:
            raise MeshDistError("MeshSet.distance: the set was not uploaded")
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
        dist = torch.empty(n_out, dtype=torch.float64, device=dev)
        face = torch.empty(n_out, dtype=torch.int32, device=dev)
        ins = torch.empty(n_out, dtype=torch.uint8, device=dev) if inside else None
        if J == 0:
            return dist, face, (ins.bool() if inside else None)
        lib = _bind()
        ptr = lambda a: a.ctypes.data_as(c_void_p)  # noqa: E731
        jbytes = _check(int(lib.tamf_meshdist_points_workspace(J)))
        with torch.cuda.device(dev):
            jws = torch.empty(jbytes // 8 + 2, dtype=torch.float64, device=dev)
            _check(lib.tamf_meshdist_points(self._ws.data_ptr(), self.M, p.data_ptr() if P else None, P, J, ptr(mid), ptr(tr), ptr(off), ptr(ln),
                                            0 if cull else 1, jws.data_ptr(), jbytes, dist.data_ptr(), face.data_ptr(),
                                            ins.data_ptr() if inside else None, _stream_ptr(dev)))
        return dist, face, (ins.bool() if inside else None)

    def lattice(self, mesh: int, ticks, cull: bool = True):
        """ticks (R, 3) float64 -> float64 (R, R, R) on the device: element [i, j, k] = distance of (ticks[i,0], ticks[j,1], ticks[k,2])"""
        import torch

        from .hip_backend import _stream_ptr

        if self._ws is None:
            raise MeshDistError("MeshSet.lattice: the set was not uploaded")
        dev = self.device
        tk = torch.as_tensor(ticks).to(device=dev, dtype=torch.float64).contiguous()
        if tk.dim() != 2 or tk.shape[1] != 3:
            raise ValueError("ticks must be (R, 3)")
        R = int(tk.shape[0])
        out = torch.empty((max(R, 0),) * 3, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _check(_bind().tamf_meshdist_lattice(self._ws.data_ptr(), self.M, int(mesh), tk.data_ptr(), R, 0 if cull else 1, out.data_ptr(),
                                                 _stream_ptr(dev)))
        return out


def mesh_distance(verts, faces, points, inside: bool = True, cull: bool = True, device=None):
    """points (P, 3) float32 against one mesh, as they are (identity pose) -> dist (P,), face (P,), inside (P,) or None"""
    return MeshSet([(verts, faces)], device=device).distance(points, [0], inside=inside, cull=cull)


def lattice_distance(verts, faces, ticks, cull: bool = True, device=None):
    """-> float64 (R, R, R): the distance of every lattice point (ticks[i,0], ticks[j,1], ticks[k,2]) to the mesh"""
    import torch

    if device is None and isinstance(ticks, torch.Tensor) and ticks.is_cuda:
        device = ticks.device
    return MeshSet([(verts, faces)], device=device).lattice(0, ticks, cull=cull)


def sdf_fields(verts, ax: Dict, dist: np.ndarray, mask: np.ndarray, bbox_expand_ratio: float, resolution: int) -> Tuple[Dict, Dict]:
    """The twelve SDFData fields from the mesh's vertices, lattice_axes' dict, the distances (R^3,) and the inside mask (R^3,): the
    numpy lines of process_sdf (sdf_util.py:60-99) with `sdf = where(mask, +dist, -dist)` in place of pysdf's values.
    -> (fields, {"n_inside", "n_surface_points"})"""
    from .metrics.siv import _aabb_corners

    v = np.asarray(verts, dtype=np.float64)
    center = ax["mesh_center"]
    aabb = _aabb_corners(v.min(axis=0), v.max(axis=0))
    aabb_centered = aabb - center
    aabb_centered_expanded = aabb_centered * bbox_expand_ratio
    ticks = ax["ticks"]
    x, y, z = np.meshgrid(ticks[:, 0], ticks[:, 1], ticks[:, 2], indexing="ij")
    query = np.vstack((x.flatten(), y.flatten(), z.flatten())).T
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    dist = np.asarray(dist, dtype=np.float64).reshape(-1)
    sdf = np.where(mask, dist, -dist)
    fields = {"mesh_center": center, "bbox": aabb, "bbox_centered": aabb_centered, "bbox_centered_expanded": aabb_centered_expanded,
              "bbox_expanded": aabb_centered_expanded + center, "bbox_expand_ratio": bbox_expand_ratio, "resolution": resolution,
              "extent": ax["extent"], "extent_expanded": ax["extent_expanded"], "tick_unit": ax["tick_unit"], "point": query + center, "sdf": sdf}
    return fields, {"n_inside": int(mask.sum()), "n_surface_points": int((mask & (dist == 0)).sum())}


def process_sdf(verts, faces, bbox_expand_ratio: float = 1.2, resolution: int = 100, device=None, cull: bool = True, info: bool = False,
                sign: str = "parity"):
    """The reference's process_sdf without pysdf: the dict of all twelve SDFData fields (SDF_FIELDS; `SDFData(**fields)` takes it).
    The numpy-line fields are those of metrics/siv.lattice_axes; `sdf` = +dist where geometry.voxelize_lattice says inside, -dist
    elsewhere (the reference's "negative outside"), float64; `point` = query point + mesh_center.  `sdf > 0` differs from the inside
    mask only on interior lattice points whose distance is exactly 0: with `info` the call returns (fields, {"n_inside",
    "n_surface_points"}), where n_surface_points counts exactly those.
    sign="winding": the mask is winding.lattice_winding's `inside` (|w| > 0.5, include/tamf_winding.h) - the sign for a mesh that is
    open or scanned; the distance is as before."""
    import torch

    from .geometry import voxelize_lattice
    from .metrics.siv import lattice_axes
    from .winding import check_sign, lattice_winding

    check_sign(sign)

    ax = lattice_axes(verts, bbox_expand_ratio, resolution)
    f = np.asarray(faces)
    tk = torch.from_numpy(np.ascontiguousarray(ax["ticks"]))
    if device is not None:
        tk = tk.to(device)
    mask = voxelize_lattice(ax["verts_centred"], f, tk) if sign == "parity" else lattice_winding(ax["verts_centred"], f, tk, device=device)[1]
    dist = lattice_distance(ax["verts_centred"], f, tk, cull=cull, device=mask.device)
    fields, extra = sdf_fields(verts, ax, dist.reshape(-1).cpu().numpy(), mask.reshape(-1).cpu().numpy(), bbox_expand_ratio, resolution)
    return (fields, extra) if info else fields


__all__ = ["TILE", "SDF_FIELDS", "MeshDistError", "MeshSet", "mesh_distance", "lattice_distance", "process_sdf", "sdf_fields", "valid_faces",
           "in_range_faces", "morton_codes", "morton_permutation", "contains_rescaling"]
