"""Point clouds from an object's surface: the bit-defined HIP surface sampler of libtamf_surface.so (include/tamf_surface.h holds the
definition) followed by farthest-point sampling with the point encoder's FPS kernel (tamf_pointenc_fps, include/tamf_pointenc.h).
The same mesh, seed and key give the same cloud on every machine.

    sample_surface(verts, faces, n, ...)      n area-uniform surface samples (points, optionally normals and face indices)
    sample_point_cloud(verts, faces, ...)     n_points * oversample samples thinned to n_points by FPS from sample 0, in FPS order
    resample_points(points, n_points, ...)    the same thinning for a scan: FPS straight away up to 32768 points, above that a Philox
                                              draw of 32768 distinct points first
    object_key(obj_id)                        the Philox key of an object: FNV-1a, 64 bit, of the id's UTF-8 bytes

How the published OakInk2 clouds were sampled is not known; these clouds are this package's own."""
from __future__ import annotations

from ctypes import c_char_p, c_int32, c_int64, c_uint64, c_void_p

import numpy as np

FPS_MAX_POINTS = 32768  # the FPS kernel's limit (model/point_encoder.py:N_MAX)
MAX_FACES = 1 << 26
MAX_SAMPLES = 2 ** 31 - 1


class SurfaceError(RuntimeError):
    pass


_lib = None


def _bind():
    global _lib
    if _lib is None:
        from . import _lib as L

        lib = L.load_surface()
        lib.tamf_surface_last_error.restype = c_char_p
        lib.tamf_surface_workspace_bytes.restype = c_int64
        lib.tamf_surface_workspace_bytes.argtypes = [c_int32]
        lib.tamf_surface_sample.argtypes = [c_void_p, c_void_p, c_int32, c_int32, c_int64, c_uint64, c_uint64, c_int64, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_int64, c_void_p]
        _lib = lib
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        raise SurfaceError(f"libtamf_surface: {_bind().tamf_surface_last_error().decode()} (status {rc})")


def object_key(obj_id: str) -> int:
    """FNV-1a, 64 bit, over the UTF-8 bytes of `obj_id`: the `key` an object's samples are drawn under (stable across runs, machines
    and Python versions, unlike the built-in hash)"""
    h = 0xCBF29CE484222325
    for b in str(obj_id).encode("utf-8"):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _u64(name: str, value) -> int:
    v = int(value)
    if not 0 <= v < 2 ** 64:
        raise ValueError(f"{name} = {v} outside [0, 2^64)")
    return v


def _mesh_arrays(verts, faces):
    """host-checked (verts float32 (V, 3), faces int32 (F, 3)) as numpy"""
    import torch

    v = verts.detach().cpu().numpy() if isinstance(verts, torch.Tensor) else np.asarray(verts)
    f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1:
        raise ValueError(f"verts: expected (V, 3) with V >= 1, got {v.shape}")
    if f.ndim != 2 or f.shape[1] != 3 or not 1 <= f.shape[0] <= MAX_FACES or f.dtype.kind not in "iu":
        raise ValueError(f"faces: expected integers of shape (F, 3) with 1 <= F <= 2^26, got {f.dtype} {f.shape}")
    if int(f.min()) < 0 or int(f.max()) >= v.shape[0]:
        bad = int(np.flatnonzero(((f < 0) | (f >= v.shape[0])).any(1))[0])
        raise ValueError(f"faces: face {bad} = {f[bad].tolist()} has an index outside [0, {v.shape[0]})")
    return np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32)


def sample_surface(verts, faces, n, seed=0, key=0, first_sample=0, normals=False, faces_out=False, device=None):
    """Samples first_sample .. first_sample + n - 1 of the mesh (include/tamf_surface.h): points (n, 3) float32 on the device, and
    with `normals` / `faces_out` a tuple (points[, normals (n, 3) float32][, face index (n,) int64]).  Face indices are range-checked
    here, on the host.  A mesh without a face of positive area raises SurfaceError.  Waits for the stream once (the total area)."""
    import torch

    from .hip_backend import _stream_ptr, require_gpu

    v, f = _mesh_arrays(verts, faces)
    n = int(n)
    if not 1 <= n <= MAX_SAMPLES:
        raise ValueError(f"n = {n} outside [1, 2^31 - 1]")
    if int(first_sample) < 0:
        raise ValueError(f"first_sample = {first_sample} is negative")
    seed, key = _u64("seed", seed), _u64("key", key)
    device = require_gpu(device)
    lib = _bind()
    with torch.cuda.device(device):
        vd, fd = torch.from_numpy(v).to(device), torch.from_numpy(f).to(device)
        points = torch.empty((n, 3), dtype=torch.float32, device=device)
        nrm = torch.empty((n, 3), dtype=torch.float32, device=device) if normals else None
        fidx = torch.empty((n,), dtype=torch.int32, device=device) if faces_out else None
        nbytes = int(lib.tamf_surface_workspace_bytes(f.shape[0]))
        if nbytes < 0:
            _check(nbytes)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
        _check(lib.tamf_surface_sample(vd.data_ptr(), fd.data_ptr(), v.shape[0], f.shape[0], n, seed, key, int(first_sample), points.data_ptr(),
                                       nrm.data_ptr() if normals else None, fidx.data_ptr() if faces_out else None, ws.data_ptr(), nbytes,
                                       _stream_ptr(device)))
    out = (points,) + ((nrm,) if normals else ()) + ((fidx.long(),) if faces_out else ())
    return out[0] if len(out) == 1 else out


def _check_counts(n_points: int, n_candidates: int, what: str) -> None:
    if n_points < 1:
        raise ValueError(f"n_points = {n_points} must be at least 1")
    if n_candidates > FPS_MAX_POINTS:
        raise ValueError(f"{what} = {n_candidates} candidates, the FPS kernel takes at most {FPS_MAX_POINTS}")


def sample_point_cloud(verts, faces, n_points=8192, oversample=4, seed=0, key=0, normals=False, faces_out=False, device=None):
    """n_points * oversample surface samples (samples 0 ..), of which n_points are kept by farthest-point sampling from sample 0
    (tamf_pointenc_fps: its float32 distance, the lowest index among equals), returned in FPS order: points (n_points, 3) float32 on
    the device, or a tuple (points[, normals][, face index]) as sample_surface.  n_points * oversample <= 32768."""
    from .model.point_encoder import fps_indices

    n_points, oversample = int(n_points), int(oversample)
    if oversample < 1:
        raise ValueError(f"oversample = {oversample} must be at least 1")
    _check_counts(n_points, n_points * oversample, f"n_points * oversample = {n_points} * {oversample}")
    got = sample_surface(verts, faces, n_points * oversample, seed=seed, key=key, normals=normals, faces_out=faces_out, device=device)
    got = got if isinstance(got, tuple) else (got,)
    keep = fps_indices(got[0], n_points, 0)
    out = tuple(t[keep] for t in got)
    return out[0] if len(out) == 1 else out


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 (Salmon et al. 2011) on uint32 numpy arrays: the generator of csrc/tamf_device.h on the host"""
    c = [np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)]
    mask = np.uint64(0xFFFFFFFF)
    for r in range(10):
        a, b = np.uint64((k0 + r * 0x9E3779B9) & 0xFFFFFFFF), np.uint64((k1 + r * 0xBB67AE85) & 0xFFFFFFFF)
        p0, p1 = c[0] * np.uint64(0xD2511F53), c[2] * np.uint64(0xCD9E8D57)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ a, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ b, p0 & mask]
    return tuple(x.astype(np.uint32) for x in c)


def draw_face_uniform(first: int, count: int, seed: int, key: int) -> np.ndarray:
    """u_f of samples first .. first + count - 1 (include/tamf_surface.h, Draw): float64, (((r0 << 21) | (r1 >> 11)) + 0.5) * 2^-53"""
    i = np.arange(first, first + count, dtype=np.uint64)
    n = np.ones(count, dtype=np.uint64)
    r0, r1, _, _ = philox4x32_10(i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), n * np.uint64(key & 0xFFFFFFFF), n * np.uint64(key >> 32),
                                 seed & 0xFFFFFFFF, seed >> 32)
    k = (r0.astype(np.uint64) << np.uint64(21)) | (r1.astype(np.uint64) >> np.uint64(11))
    return (k.astype(np.float64) + 0.5) * 2.0 ** -53


def thin_indices(n: int, keep: int, seed=0, key=0) -> np.ndarray:
    """`keep` distinct indices of range(n), keep <= n: min(floor(u_f * n), n - 1) of the Philox draws 0, 1, 2, ... under (seed, key)
    (draw_face_uniform), every index at its first occurrence, in draw order, until `keep` are held"""
    if not 1 <= keep <= n:
        raise ValueError(f"cannot keep {keep} of {n}")
    seed, key = _u64("seed", seed), _u64("key", key)
    taken = np.zeros(n, dtype=bool)
    out, first = [], 0
    have = 0
    while have < keep:
        count = max(4096, 2 * (keep - have))
        idx = np.minimum(np.floor(draw_face_uniform(first, count, seed, key) * float(n)).astype(np.int64), n - 1)
        first += count
        _, pos = np.unique(idx, return_index=True)  # first occurrence of every index of this batch, then those not yet taken
        pos = np.sort(pos)
        new = idx[pos][~taken[idx[pos]]][: keep - have]
        taken[new] = True
        out.append(new)
        have += new.shape[0]
    return np.concatenate(out)


def resample_points(points, n_points, seed=0, key=0, device=None, indices_out=False):
    """A scan thinned to n_points by farthest-point sampling from its first point, in FPS order: (n_points, 3) float32 on the device
    (with `indices_out` also the rows of `points` they are).  More than 32768 points are first thinned to 32768 by thin_indices(N,
    32768, seed, key), in draw order; seed and key play no part below that.  Fewer than n_points points is refused."""
    import torch

    from .hip_backend import require_gpu
    from .model.point_encoder import fps_indices

    p = points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else np.asarray(points)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"points: expected (N, 3), got {p.shape}")
    p = np.ascontiguousarray(p, dtype=np.float32)
    if not np.isfinite(p).all():
        raise ValueError("points: holds a non-finite value")
    n_points = int(n_points)
    _check_counts(n_points, n_points, "n_points")
    if p.shape[0] < n_points:
        raise ValueError(f"points: {p.shape[0]} points, fewer than the {n_points} asked for")
    rows = np.arange(p.shape[0], dtype=np.int64)
    if p.shape[0] > FPS_MAX_POINTS:
        rows = thin_indices(p.shape[0], FPS_MAX_POINTS, seed, key)
    device = require_gpu(device)
    cand = torch.from_numpy(p[rows]).to(device)
    keep = fps_indices(cand, n_points, 0)
    out = cand[keep]
    return (out, torch.from_numpy(rows).to(device)[keep]) if indices_out else out


__all__ = ["SurfaceError", "FPS_MAX_POINTS", "object_key", "sample_surface", "sample_point_cloud", "resample_points", "thin_indices",
           "draw_face_uniform", "philox4x32_10"]
