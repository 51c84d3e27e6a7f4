"""include/tamf_surface.h restated in numpy float64, the reference of the surface sampler's tests: areas, the CDF by a sequential
np.cumsum, the Philox draws through oracle.mdm_oracle.philox4x32_10, the face pick by np.searchsorted(side="right"), point and normal
as defined, FPS by tests/pointenc_fixture.host_fps.  numpy evaluates every product and sum on its own (no fused multiply-add).

The library sums the CDF in another (fixed) order, so a sample whose u_f * total falls within the two summations' error of a CDF step
may land on the neighbouring face.  `sample` marks those: `near[i]` is true when |u_f total - cdf[j]| <= F 2^-52 total for the step
below or above the pick - computed from THIS CDF, never from the library's.  Also the test meshes."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import mdm_oracle as O  # noqa: E402

SCAN_BLOCK = 1024  # TAMF_SURFACE_SCAN_BLOCK


def areas_and_cross(verts, faces):
    """(area (F,), c (F, 3)) float64; a face with an index outside [0, V) or a non-finite area has area 0"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < v.shape[0])).all(1)
    g = np.where(ok[:, None], f, 0)
    e1, e2 = v[g[:, 1]] - v[g[:, 0]], v[g[:, 2]] - v[g[:, 0]]
    with np.errstate(all="ignore"):
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        area = 0.5 * np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    area = np.where(ok & np.isfinite(area), area, 0.0)
    return area, c


def draws(first: int, count: int, seed: int, key: int):
    """(u_f, u_1, u_2) float64 of samples first .. first + count - 1"""
    i = np.arange(first, first + count, dtype=np.uint64)
    full = lambda x: np.full(count, x, dtype=np.uint32)  # noqa: E731
    r0, r1, r2, r3 = O.philox4x32_10((i & np.uint64(0xFFFFFFFF)).astype(np.uint32), (i >> np.uint64(32)).astype(np.uint32),
                                     full(key & 0xFFFFFFFF), full((key >> 32) & 0xFFFFFFFF), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    k = (r0.astype(np.uint64) << np.uint64(21)) | (r1.astype(np.uint64) >> np.uint64(11))
    return (k.astype(np.float64) + 0.5) * 2.0 ** -53, (r2.astype(np.float64) + 0.5) * 2.0 ** -32, (r3.astype(np.float64) + 0.5) * 2.0 ** -32


def sample(verts, faces, n: int, seed: int = 0, key: int = 0, first_sample: int = 0):
    """-> dict: face (n,) int64, point (n, 3) float32, normal (n, 3) float32, point64 / weights (n, 3) float64, near (n,) bool, cdf,
    total"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = f.shape[0]
    area, c = areas_and_cross(verts, faces)
    cdf = np.cumsum(area)  # sequential, float64
    total = float(cdf[-1])
    assert total > 0 and np.isfinite(total)
    uf, u1, u2 = draws(first_sample, n, seed, key)
    x = uf * total
    j = np.searchsorted(cdf, x, side="right")
    j = np.where(j >= F, np.searchsorted(cdf, total, side="left"), j)
    tol = F * 2.0 ** -52 * total
    below = np.where(j > 0, cdf[np.maximum(j - 1, 0)], -np.inf)  # the step the pick lies above (none for face 0: x >= 0 always holds)
    near = (np.abs(x - below) <= tol) | ((np.abs(x - cdf[j]) <= tol) & (cdf[j] < total))
    s = np.sqrt(u1)
    w = np.stack([1.0 - s, s * (1.0 - u2), s * u2], 1)
    tri = v[f[j]]  # (n, 3, 3)
    p64 = (w[:, 0:1] * tri[:, 0] + w[:, 1:2] * tri[:, 1]) + w[:, 2:3] * tri[:, 2]
    cj = c[j]
    nrm = cj / np.sqrt((cj[:, 0] * cj[:, 0] + cj[:, 1] * cj[:, 1]) + cj[:, 2] * cj[:, 2])[:, None]
    return {"face": j.astype(np.int64), "point": p64.astype(np.float32), "normal": nrm.astype(np.float32), "point64": p64, "weights": w,
            "near": near, "cdf": cdf, "total": total, "area": area}


def point_cloud(verts, faces, n_points: int, oversample: int, seed: int = 0, key: int = 0):
    """sample_point_cloud restated: -> (kept sample indices (n_points,) in FPS order, the restated samples)"""
    from pointenc_fixture import host_fps

    r = sample(verts, faces, n_points * oversample, seed, key)
    return host_fps(r["point"], n_points, 0)[0], r


def thin(n: int, keep: int, seed: int = 0, key: int = 0) -> np.ndarray:
    """thin_indices restated draw by draw: min(floor(u_f n), n - 1), first occurrences in draw order until `keep` are held"""
    out, seen, first = [], set(), 0
    while len(out) < keep:
        uf = draws(first, 8192, seed, key)[0]
        first += 8192
        for i in np.minimum(np.floor(uf * float(n)).astype(np.int64), n - 1).tolist():
            if i not in seen:
                seen.add(i)
                out.append(i)
                if len(out) == keep:
                    break
    return np.asarray(out, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------
# meshes of the tests
# ---------------------------------------------------------------------------------------------------------------------------------
def triangle():
    return np.array([[0.1, 0.2, 0.3], [1.3, 0.1, -0.2], [0.4, 1.1, 0.7]], np.float32), np.array([[0, 1, 2]], np.int32)


def tetrahedron():
    v = np.array([[0.0, 0.0, 0.0], [0.11, 0.01, 0.0], [0.02, 0.13, 0.01], [0.03, 0.02, 0.17]], np.float32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)


def cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32) * np.float32(0.1) - np.float32(0.03)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return v.astype(np.float32), f


def broken_cube():
    """the cube with two zero-area faces (a repeated index; three points on a line) and one face with an index past the vertices:
    for the C entry point only (sample_surface refuses the index on the host)"""
    v, f = cube()
    v = np.concatenate([v, ((v[0] + v[1]) * np.float32(0.5))[None]]).astype(np.float32)  # vertex 8: the middle of edge 0-1
    extra = np.array([[3, 3, 5], [0, 8, 1], [0, 1, 9]], np.int32)
    return v, np.concatenate([f[:5], extra[:2], f[5:], extra[2:]]).astype(np.int32)


def icosphere(subdivisions: int = 3, radius: float = 0.05):
    """20 * 4^subdivisions faces (1 280 at 3)"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius + np.array([0.01, -0.02, 0.03])).astype(np.float32), np.asarray(f, np.int32)


def strip(n_faces: int, lo: float = 1.0, hi: float = 1.0):
    """n_faces separate right triangles in a row whose areas run geometrically from `lo` to `hi` (legs sqrt(2 area))"""
    a = np.geomspace(lo, hi, n_faces) if n_faces > 1 else np.array([lo])
    leg = np.sqrt(2.0 * a)
    x0 = np.concatenate([[0.0], np.cumsum(leg[:-1] + 0.01)])
    v = np.zeros((n_faces, 3, 3))
    v[:, :, 0] = x0[:, None]
    v[:, 1, 0] += leg
    v[:, 2, 1] = leg
    v[:, :, 2] = 0.25
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)


# name -> (verts, faces); every sample count of SAMPLE_COUNTS is drawn from each with seed SEED and key KEY
SAMPLE_COUNTS = (1, 63, 64, 65, 4096)
SEED, KEY = 20240607, 0x0123456789ABCDEF


def gpu_meshes():
    return {
        "triangle": triangle(), "tetrahedron": tetrahedron(), "broken_cube": broken_cube(), "icosphere": icosphere(3),
        "strip_1e-12": strip(40, 1e-12, 1.0),
        "block-1": strip(SCAN_BLOCK - 1, 0.5, 2.0), "block": strip(SCAN_BLOCK, 0.5, 2.0), "block+1": strip(SCAN_BLOCK + 1, 0.5, 2.0),
        "2blocks+1": strip(2 * SCAN_BLOCK + 1, 0.5, 2.0),
    }
