"""numpy restatement of the definition in include/tamf_meshdist.h: the exact point-to-mesh distance, vectorised over faces x points,
float64, the header's region order and operation order (numpy never fuses a multiply with an add).  The yardstick of the GPU tests;
it also returns the closest point and the region, which the library does not."""
import numpy as np


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def valid_faces(verts, faces):
    """bool (F,): indices in [0, V), pairwise different, area by mesh_io.face_areas > 0"""
    from oakink2_tamf_amd.mesh_io import face_areas

    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < v.shape[0])).all(1)
    ok &= (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    area = np.zeros(f.shape[0])
    area[ok] = face_areas(v, f[ok])
    return ok & (area > 0)


def closest_on_triangles(a, b, c, p):
    """a, b, c (F, 3), p (P, 3) -> q (F, P, 3), d2 (F, P), region (F, P) in 0 .. 6 = A, B, AB, C, AC, BC, interior"""
    a, b, c = (np.asarray(x, dtype=np.float64)[:, None, :] for x in (a, b, c))
    p = np.asarray(p, dtype=np.float64)[None, :, :]
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        ap = p - a
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = p - b
        d3, d4 = dot(ab, bp), dot(ac, bp)
        cp = p - c
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        k = np.full(d1.shape, 6, dtype=np.int64)
        k = np.where((va <= 0) & (e43 >= 0) & (e56 >= 0), 5, k)
        k = np.where((vb <= 0) & (d2 >= 0) & (d6 <= 0), 4, k)
        k = np.where((d6 >= 0) & (d5 <= d6), 3, k)
        k = np.where((vc <= 0) & (d1 >= 0) & (d3 <= 0), 2, k)
        k = np.where((d3 >= 0) & (d4 <= d3), 1, k)
        k = np.where((d1 <= 0) & (d2 <= 0), 0, k)
        shape = d1.shape + (3,)
        A, B, C = (np.broadcast_to(x, shape) for x in (a, b, c))
        AB, AC = np.broadcast_to(ab, shape), np.broadcast_to(ac, shape)
        v_ab = (d1 / (d1 - d3))[..., None]
        w_ac = (d2 / (d2 - d6))[..., None]
        w_bc = (e43 / (e43 + e56))[..., None]
        denom = 1.0 / ((va + vb) + vc)
        v_in, w_in = (vb * denom)[..., None], (vc * denom)[..., None]
        kk = k[..., None]
        q = (A + AB * v_in) + AC * w_in
        q = np.where(kk == 5, B + (C - B) * w_bc, q)
        q = np.where(kk == 4, A + AC * w_ac, q)
        q = np.where(kk == 3, C, q)
        q = np.where(kk == 2, A + AB * v_ab, q)
        q = np.where(kk == 1, B, q)
        q = np.where(kk == 0, A, q)
        d = p - q
        return q, dot(d, d), k


def mesh_distance(verts, faces, points, chunk=None):
    """-> dist (P,) f64, face (P,) int32 (original index; -1 when nothing wins), closest point (P, 3), d2 (P,)"""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    idx = np.flatnonzero(valid_faces(v, f))
    assert idx.size, "no valid face"
    a, b, c = v[f[idx, 0]], v[f[idx, 1]], v[f[idx, 2]]
    P = p.shape[0]
    chunk = max(1, 400000 // idx.size) if chunk is None else chunk
    dist, face, close, dd = np.empty(P), np.empty(P, np.int32), np.empty((P, 3)), np.empty(P)
    for s in range(0, P, chunk):
        q, d2, _ = closest_on_triangles(a, b, c, p[s:s + chunk])
        with np.errstate(all="ignore"):
            best = np.where(np.isnan(d2), np.inf, d2).min(axis=0)  # (the minimum of the values; a NaN never wins)
        attain = d2 == best[None, :]
        first = attain.argmax(axis=0)  # (idx ascends: the first row that attains it has the lowest original index)
        n = np.arange(q.shape[1])
        none = ~attain.any(axis=0)
        dd[s:s + chunk] = best
        dist[s:s + chunk] = np.sqrt(best)
        face[s:s + chunk] = np.where(none, -1, idx[first])
        close[s:s + chunk] = q[first, n]
    return dist, face, close, dd


def query_points(points_f32, transf):
    """the header's query point: ((R00 x + R01 y) + R02 z) + t0 of the float32 point widened exactly; transf (12,) or (3, 4)"""
    x = np.asarray(points_f32, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(transf, dtype=np.float64).reshape(3, 4)
    return np.stack([((t[r, 0] * x[:, 0] + t[r, 1] * x[:, 1]) + t[r, 2] * x[:, 2]) + t[r, 3] for r in range(3)], axis=1)


def lattice_points(ticks):
    """(R, 3) -> (R^3, 3), index (i R + j) R + k"""
    t = np.asarray(ticks, dtype=np.float64)
    g = np.meshgrid(t[:, 0], t[:, 1], t[:, 2], indexing="ij")
    return np.stack([x.reshape(-1) for x in g], axis=1)
