"""Meshes and point sets shared by the point-to-mesh distance tests (CPU and GPU): small ones built here, and the meshes inside the
tests/golden/siv_lattice_*.npz fixtures."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE = 64
FIXTURES = ("sphere", "torus", "rotbox", "aabox", "twoparts")


@functools.lru_cache(maxsize=None)
def fixture_mesh(name):
    with np.load(os.path.join(GOLDEN, f"siv_lattice_{name}.npz")) as z:
        return np.array(z["verts"], dtype=np.float64), np.array(z["faces"], dtype=np.int32)


def flat_grid(n_faces, step=0.125):
    """n_faces right triangles with legs `step` (a power of two) in the plane z = 0.25: every coordinate, edge midpoint and the
    interior point a/2 + b/4 + c/4 is a float32 number, and the closest-point arithmetic on them is exact"""
    cols = 8
    rows = (n_faces + 2 * cols - 1) // (2 * cols)
    ii, jj = np.meshgrid(np.arange(rows + 1), np.arange(cols + 1), indexing="ij")
    verts = np.stack([ii.reshape(-1) * step, jj.reshape(-1) * step, np.full(ii.size, 0.25)], axis=1)
    faces = []
    for i in range(rows):
        for j in range(cols):
            a, b, c, d = i * (cols + 1) + j, i * (cols + 1) + j + 1, (i + 1) * (cols + 1) + j, (i + 1) * (cols + 1) + j + 1
            faces += [[a, b, c], [b, d, c]]
    return verts, np.asarray(faces[:n_faces], dtype=np.int32)


def bumpy_grid(n_faces, seed=3):
    """flat_grid with random heights: a surface whose closest points fall into all seven regions"""
    v, f = flat_grid(n_faces)
    v = v.copy()
    v[:, 2] = np.random.default_rng(seed).uniform(0.0, 0.2, v.shape[0])
    return v, f


def confetti(n_faces=200, seed=5):
    """random large triangles in the unit cube: every tile's box is nearly the whole cube, a point in it lies in many boxes at once"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.2, 0.8, (n_faces, 1, 3))
    verts = (c + rng.uniform(-0.3, 0.3, (n_faces, 3, 3))).reshape(-1, 3)
    return verts, np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)


def with_invalid_faces(verts, faces):
    """the mesh with a repeated-index face, a zero-area face (three collinear vertices, appended) and an out-of-range index mixed
    in: -> verts, faces, the rows of the bad faces"""
    v = np.concatenate([verts, [[2.0, 2.0, 2.0], [3.0, 3.0, 3.0], [4.0, 4.0, 4.0]]])
    V = v.shape[0]
    f = np.asarray(faces, dtype=np.int32)
    bad = np.asarray([[f[0, 0], f[0, 0], f[0, 1]], [V - 3, V - 2, V - 1], [f[1, 0], f[1, 1], V + 5], [f[2, 0], -1, f[2, 2]]], dtype=np.int32)
    out = np.concatenate([f[:3], bad[:2], f[3:10], bad[2:], f[10:]])
    return v, out, [3, 4, 12, 13]


def points_around(verts, n, seed, expand=1.5):
    """float32 (n, 3) uniform in the mesh's bounding box grown by `expand` about its centre"""
    v = np.asarray(verts, dtype=np.float64)
    lo, hi = v.min(0), v.max(0)
    c, h = (lo + hi) / 2, np.maximum((hi - lo) / 2, 0.05) * expand
    return np.random.default_rng(seed).uniform(c - h, c + h, (n, 3)).astype(np.float32)


def on_surface_points(verts, faces):
    """float32 points exactly on flat_grid's vertices, edge midpoints and face interiors: (points, kind) with kind 0 / 1 / 2"""
    v, f = np.asarray(verts, dtype=np.float64), np.asarray(faces)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    used = v[np.unique(f)]
    pts = np.concatenate([used, (a + b) / 2, (b + c) / 2, (a + c) / 2, a / 2 + b / 4 + c / 4])
    kind = np.concatenate([np.zeros(len(used)), np.ones(3 * len(f)), np.full(len(f), 2)]).astype(np.int64)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    return pts.astype(np.float32), kind


def rigid(seed, scale_t=0.3):
    """a (3, 4) float64 [R | t] with a proper rotation that is far from the identity"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return np.concatenate([q, rng.uniform(-scale_t, scale_t, (3, 1))], axis=1)


IDENTITY = np.eye(3, 4)
