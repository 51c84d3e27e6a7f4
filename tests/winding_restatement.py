"""include/tamf_winding.h restated in numpy: the valid-face predicate of tamf_meshdist.h, van Oosterom and Strackee's omega per face
with the header's association, the chunked serial summation, np.arctan2.  Run in float64 it is the library's arithmetic (atan2 aside,
which the header leaves to the device library); run in np.longdouble (80-bit here) the identical arithmetic is the truth the tests'
gates are taken against."""
import numpy as np

from oakink2_tamf_amd.meshdist import valid_faces

CHUNK = 1024
FOUR_PI = 12.566370614359172


def require_longdouble():
    """the longdouble run is the truth only when it is wider than float64: fail, not skip, otherwise"""
    assert np.finfo(np.longdouble).nmant >= 63, f"np.longdouble has {np.finfo(np.longdouble).nmant} mantissa bits: no wider than float64 here"


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def omega(tri, p, dtype=np.float64):
    """tri (F, 3, 3) vertices of the faces, p (P, 3) -> (P, F) solid angles in `dtype`"""
    tri = np.asarray(tri, dtype=np.float64).astype(dtype)
    p = np.asarray(p, dtype=np.float64).astype(dtype)
    a = [tri[None, :, 0, k] - p[:, None, k] for k in range(3)]
    b = [tri[None, :, 1, k] - p[:, None, k] for k in range(3)]
    c = [tri[None, :, 2, k] - p[:, None, k] for k in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
        cr = [b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]]
        det = _dot(a, cr)
        den = ((la * lb) * lc + _dot(a, b) * lc) + (_dot(b, c) * la + _dot(c, a) * lb)
        return dtype(2.0) * np.arctan2(det, den)


def transform(points, transf=None, dtype=np.float64):
    """the header's query point: float32 points widened exactly, through rows [R | t] (None: as they are)"""
    p = np.asarray(points)
    assert p.dtype == np.float32
    p = p.reshape(-1, 3).astype(dtype)
    if transf is None:
        return p
    t = np.asarray(transf, dtype=np.float64).reshape(12).astype(dtype)
    with np.errstate(invalid="ignore"):
        return np.stack([((t[4 * r] * p[:, 0] + t[4 * r + 1] * p[:, 1]) + t[4 * r + 2] * p[:, 2]) + t[4 * r + 3] for r in range(3)], axis=1)


def winding(verts, faces, p, dtype=np.float64, batch=4096):
    """w (P,) in `dtype` of the query points p (P, 3) (float64 values; see transform): chunks of CHUNK valid faces in ascending index,
    serial sums from +0 inside a chunk and over the chunks, divided by the float64 nearest to 4 pi"""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    idx = np.flatnonzero(valid_faces(v, f))
    tri = v[f[idx]]
    p = np.asarray(p).reshape(-1, 3)
    out = np.zeros(p.shape[0], dtype=dtype)
    for s in range(0, p.shape[0], batch):
        q = p[s:s + batch]
        total = np.zeros(q.shape[0], dtype=dtype)
        for c0 in range(0, len(idx), CHUNK):
            om = omega(tri[c0:c0 + CHUNK], q, dtype)
            part = np.zeros(q.shape[0], dtype=dtype)
            for k in range(om.shape[1]):
                part = part + om[:, k]
            total = total + part
        out[s:s + batch] = total / dtype(FOUR_PI)
    return out


def inside(w):
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(w)) > 0.5


def n_valid(verts, faces):
    return int(valid_faces(np.asarray(verts, dtype=np.float64), np.asarray(faces)).sum())


def truth_and_gate(verts, faces, p):
    """-> (w64, truth (longdouble), gate): gate = max(4 e_ref, F 2^-53), e_ref the largest |float64 - longdouble| restatement over
    these points (NaN rows left out), F the number of valid faces"""
    require_longdouble()
    w64 = winding(verts, faces, p, np.float64)
    wl = winding(verts, faces, p, np.longdouble)
    d = np.abs(w64.astype(np.longdouble) - wl)
    e_ref = float(np.nanmax(d)) if np.isfinite(d).any() else 0.0
    return w64, wl, max(4.0 * e_ref, n_valid(verts, faces) * 2.0 ** -53)


def lattice_points(ticks):
    """(R^3, 3) in the kernels' order: element (i R + j) R + k = (ticks[i,0], ticks[j,1], ticks[k,2])"""
    t = np.asarray(ticks, dtype=np.float64)
    x, y, z = np.meshgrid(t[:, 0], t[:, 1], t[:, 2], indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)


# ---- meshes of the tests --------------------------------------------------------------------------------------------------------------
def cube(half=0.5, centre=(0.0, 0.0, 0.0)):
    """the closed cube, 12 outward faces; faces 10 and 11 are its top (+z)"""
    c = np.asarray(centre, dtype=np.float64)
    v = np.asarray([[x, y, z] for x in (-half, half) for y in (-half, half) for z in (-half, half)], dtype=np.float64) + c
    f = np.asarray([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                    [1, 5, 7], [1, 7, 3]], dtype=np.int32)
    return v, f


def open_cube(half=0.5, centre=(0.0, 0.0, 0.0)):
    """the cube without its top (+z) face"""
    v, f = cube(half, centre)
    return v, f[:10]


def uv_sphere(n_lat=16, n_lon=32, radius=0.05):
    """closed UV sphere with its poles on z: 2 + (n_lat - 1) n_lon vertices, 2 n_lon (n_lat - 1) faces, outward"""
    verts = [[0.0, 0.0, radius]]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            verts.append([radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)])
    verts.append([0.0, 0.0, -radius])
    ring = lambda i, j: 1 + (i - 1) * n_lon + (j % n_lon)  # noqa: E731
    faces = []
    for j in range(n_lon):
        faces.append([0, ring(1, j), ring(1, j + 1)])
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            faces.append([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)])
            faces.append([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)])
    south = len(verts) - 1
    for j in range(n_lon):
        faces.append([south, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)])
    return np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int32)


def inscribed_radius(verts, faces):
    """the smallest distance from the origin to a face's plane: the radius of the largest ball about the origin inside a convex
    polyhedron that contains it"""
    v = np.asarray(verts, dtype=np.float64)
    tri = v[np.asarray(faces)]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return float(np.abs((n * tri[:, 0]).sum(1)).min())


def sphere_lattice(radius=0.05, R=24, expand=1.2):
    """(R, 3) float64 ticks of an R^3 lattice over [-expand radius, expand radius]^3, rounded to float32 values"""
    t = np.linspace(-expand * radius, expand * radius, R).astype(np.float32).astype(np.float64)
    return np.stack([t, t, t], axis=1)
