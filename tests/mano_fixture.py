"""Seeded MANO-shaped arrays for the tests of the native MANO layer: nothing of the (licence-gated) MANO assets, only their shapes,
their kinematic tree and their magnitudes (metres)."""
import numpy as np

PARENTS = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]  # the published MANO tree: wrist, then five chains of three
SMALL_TIPS = (3, 7, 11, 15, 19)  # fingertip stand-ins of the V = 20 variant (the defaults are MANO's vertex ids, > 20)
SHAPES = {778: (21, 37), 20: (1, 19)}  # V -> (rings, segments): V = 1 + rings * segments


def open_sphere(rings, segs, radius=0.05):
    """UV sphere of 1 + rings * segs vertices with the north polar cap removed: pole 0 at the south, ring r at vertices
    1 + r * segs .., the last ring is the open boundary.  Outward-oriented triangles."""
    v = [(0.0, 0.0, -radius)]
    for r in range(rings):
        th = np.pi * (r + 1) / (rings + 2)  # polar angle from the south pole; stops short of the north pole
        for s in range(segs):
            ph = 2 * np.pi * s / segs
            v.append((radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), -radius * np.cos(th)))
    f = []
    ring = lambda r, s: 1 + r * segs + s % segs  # noqa: E731
    for s in range(segs):
        f.append((0, ring(0, s + 1), ring(0, s)))
    for r in range(rings - 1):
        for s in range(segs):
            a, b, c, d = ring(r, s), ring(r, s + 1), ring(r + 1, s), ring(r + 1, s + 1)
            f += [(a, b, d), (a, d, c)]
    return np.array(v, np.float64), np.array(f, np.int64)


def synthetic_arrays(V=778, seed=0):
    """dict of numpy arrays accepted by oakink2_tamf_amd.mano.ManoArrays(**d)"""
    rings, segs = SHAPES[V]
    rng = np.random.default_rng(1000 * seed + V)
    vt, faces = open_sphere(rings, segs)
    vt = vt * np.array([1.0, 0.6, 0.9]) + rng.normal(size=vt.shape) * 1e-3 + np.array([0.09, 0.0, 0.01])
    J_reg = np.zeros((16, V))
    for j in range(16):
        idx = rng.choice(V, size=min(12, V), replace=False)
        w = rng.random(idx.size) + 0.1
        J_reg[j, idx] = w / w.sum()
    W = np.zeros((V, 16))
    for i in range(V):
        k = int(rng.integers(1, 5))
        idx = rng.choice(16, size=k, replace=False)
        w = rng.random(k) + 0.05
        W[i, idx] = w / w.sum()
    d = dict(v_template=vt, shapedirs=rng.normal(size=(V, 3, 10)) * 1e-2, posedirs=rng.normal(size=(V, 3, 135)) * 1e-2,
             J_regressor=J_reg, weights=W, parents=np.array(PARENTS, np.int64), faces=faces)
    if V < 778:
        d["tip_ids"] = np.array(SMALL_TIPS, np.int64)
    return d


def random_inputs(N, seed=0, scale=None):
    """unit quaternions uniform over the sphere (normalised Gaussians) (N,16,4) and betas ~ N(0,1) (N,10), float64 numpy;
    `scale`: per-joint factors applied to the quaternions (non-unit input)"""
    rng = np.random.default_rng(77 + seed)
    q = rng.normal(size=(N, 16, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    if scale is not None:
        q = q * np.asarray(scale, np.float64).reshape(1, -1, 1)
    return q, rng.normal(size=(N, 10))
