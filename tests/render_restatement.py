"""The renderer's definition (include/tamf_render.h) restated in numpy: projection, triangle and point rasterisation with the depth
test, shading.  Coverage is int64 arithmetic on snapped coordinates, exactly as defined; everything real is float64 unless a dtype is
given (the float32 runs measure what fp32 arithmetic costs, for the gates of the GPU tests).  Where the library takes snapped
coordinates (raster, points, shade), so do these functions.  No torch, no GPU."""
import numpy as np

INVALID = -(2 ** 31)
SUB = 256
XY_LIMIT = 2 ** 28
NEAR_TIE = 1e-5  # relative depth gap below which two candidates of a pixel count as a near tie


def project(verts, model, view, fx, fy, cx, cy, near, F=None, dtype=np.float64):
    """verts (V,3) or (F,V,3); model (F,3,4) or None; view (3,4) -> pos_cam (F,V,3) dtype, xy (F,V,2) int64 with INVALID twice for an
    invalid vertex, uv (F,V,2) dtype: the unrounded 256 * pixel coordinates (NaN where z is not positive or the vertex is not finite)"""
    v = np.asarray(verts, dtype)
    if v.ndim == 2:
        v = np.broadcast_to(v, ((model.shape[0] if model is not None else (F or 1)),) + v.shape)
    view = np.asarray(view, dtype)
    if model is not None:
        m = np.asarray(model, dtype)
        v = np.einsum("fij,fvj->fvi", m[:, :, :3], v) + m[:, None, :, 3]
    pos = np.einsum("ij,fvj->fvi", view[:, :3], v) + view[None, None, :, 3]
    pos = pos.astype(dtype)
    z = pos[..., 2]
    ok = np.isfinite(pos).all(axis=-1) & (z >= dtype(near))
    with np.errstate(all="ignore"):
        u = (dtype(fx) * pos[..., 0] / z + dtype(cx)) * dtype(SUB)
        w = (dtype(fy) * pos[..., 1] / z + dtype(cy)) * dtype(SUB)
    uv = np.stack([u, w], axis=-1)
    snapped = np.rint(np.where(ok[..., None], uv, 0.0))  # round half to even
    ok &= (np.abs(snapped) <= XY_LIMIT).all(axis=-1)
    xy = np.where(ok[..., None], snapped, INVALID).astype(np.int64)
    return pos, xy, uv


class Buffers:
    """depth / prim_id of F frames, plus per pixel the depth of the nearest candidate that LOST the depth test (runner_up): what
    near_tie() reads, and the number of candidates that covered the pixel"""

    def __init__(self, F, H, W, dtype=np.float64):
        self.dtype = dtype
        self.depth = np.full((F, H, W), np.inf, dtype)
        self.prim_id = np.full((F, H, W), -1, np.int64)
        self.runner_up = np.full((F, H, W), np.inf, dtype)
        self.cover = np.zeros((F, H, W), np.int64)

    def offer(self, f, ys, xs, d, pid):
        """candidates in ascending primitive order: strict `<` keeps the earlier one on an exact tie"""
        sub = (f, ys, xs)
        old = self.depth[sub]
        win = d < old
        loser = np.where(win, old, d)
        self.runner_up[sub] = np.minimum(self.runner_up[sub], loser)
        self.depth[sub] = np.where(win, d, old)
        self.prim_id[sub] = np.where(win, pid, self.prim_id[sub])
        self.cover[sub] += 1

    def near_tie(self, tol=NEAR_TIE):
        with np.errstate(invalid="ignore"):
            return np.isfinite(self.runner_up) & ((self.runner_up - self.depth) <= tol * np.abs(self.runner_up))

    def near_tie_share(self):
        covered = int((self.prim_id >= 0).sum())
        return (int(self.near_tie().sum()) / covered) if covered else 0.0


def oriented(xy_f, face):
    """-> (x (3,), y (3,), vertex ids (3,), area2 > 0) python ints, or None when the triangle is dropped"""
    ids = [int(i) for i in face]
    if any(i < 0 or i >= xy_f.shape[0] for i in ids):
        return None
    x = [int(xy_f[i, 0]) for i in ids]
    y = [int(xy_f[i, 1]) for i in ids]
    if INVALID in x:
        return None
    a2 = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    if a2 == 0:
        return None
    if a2 < 0:
        x[1], x[2], y[1], y[2], ids[1], ids[2] = x[2], x[1], y[2], y[1], ids[2], ids[1]
        a2 = -a2
    return x, y, ids, a2


def edge(x, y, k):
    a, b = (k + 1) % 3, (k + 2) % 3
    return y[a] - y[b], x[b] - x[a], x[a] * y[b] - y[a] * x[b]


def edge_values(x, y, px, py):
    """E_k (int64 arrays) and the inside mask at centres px, py (int64 arrays, fixed point)"""
    E, inside = [], np.ones(np.broadcast(px, py).shape, bool)
    for k in range(3):
        A, B, C = edge(x, y, k)
        e = A * px + B * py + C
        E.append(e)
        inside &= (e > 0) | ((e == 0) & (A > 0 or (A == 0 and B < 0)))
    return E, inside


def raster(buf, xy, pos_cam, faces, prim_base=0):
    """the triangles `faces` (Nf,3) over xy (F,V,2) int, pos_cam (F,V,3), into buf"""
    F, H, W = buf.depth.shape
    dt = buf.dtype
    for f in range(F):
        z = np.asarray(pos_cam[f], dt)[:, 2]
        for t, face in enumerate(np.asarray(faces)):
            o = oriented(xy[f], face)
            if o is None:
                continue
            x, y, ids, a2 = o
            # pixel centres (256 i + 128) inside the bounding box, clipped to the image
            i0, i1 = max(0, -((-(min(x) - 128)) // SUB)), min(W - 1, (max(x) - 128) // SUB)
            j0, j1 = max(0, -((-(min(y) - 128)) // SUB)), min(H - 1, (max(y) - 128) // SUB)
            if i0 > i1 or j0 > j1:
                continue
            jj, ii = np.meshgrid(np.arange(j0, j1 + 1, dtype=np.int64), np.arange(i0, i1 + 1, dtype=np.int64), indexing="ij")
            E, inside = edge_values(x, y, ii * SUB + 128, jj * SUB + 128)
            if not inside.any():
                continue
            inv_z = sum(E[k][inside].astype(dt) / z[ids[k]] for k in range(3)) / dt(a2)
            buf.offer(f, jj[inside], ii[inside], (dt(1) / inv_z).astype(dt), prim_base + t)


def points(buf, xy, pos_cam, point_size, prim_base=0):
    """the points xy (F,P,2), pos_cam (F,P,3) as squares of point_size pixels, into buf"""
    F, H, W = buf.depth.shape
    h = point_size // 2
    for f in range(F):
        for t in range(xy.shape[1]):
            if int(xy[f, t, 0]) == INVALID:
                continue
            qx, qy = int(xy[f, t, 0]) // SUB, int(xy[f, t, 1]) // SUB  # floor
            i0, i1, j0, j1 = max(0, qx - h), min(W - 1, qx + h), max(0, qy - h), min(H - 1, qy + h)
            if i0 > i1 or j0 > j1:
                continue
            jj, ii = np.meshgrid(np.arange(j0, j1 + 1), np.arange(i0, i1 + 1), indexing="ij")
            buf.offer(f, jj.ravel(), ii.ravel(), np.full(jj.size, buf.dtype(pos_cam[f, t, 2])), prim_base + t)


def to_byte(c):
    return np.floor(255.0 * np.clip(c, 0.0, 1.0) + 0.5).astype(np.uint8)


def shade_mesh(rgb, prim_id, xy, pos_cam, normals, faces, prim_base, base, ambient, lights, dtype=np.float64):
    """writes rgb (F,H,W,3) uint8 where prim_id lies in [prim_base, prim_base + Nf); lights (L,4): unit direction, strength
    -> facing (F,H,W): |n . p| / |p| at the shaded pixels (how far the flip to the viewer is from undecided), NaN elsewhere"""
    faces = np.asarray(faces)
    F, H, W = prim_id.shape
    facing = np.full((F, H, W), np.nan)
    lights = np.asarray(lights, dtype).reshape(-1, 4)
    for f, j, i in zip(*np.nonzero((prim_id >= prim_base) & (prim_id < prim_base + faces.shape[0]))):
        o = oriented(xy[f], faces[prim_id[f, j, i] - prim_base])
        if o is None:
            continue
        x, y, ids, a2 = o
        p = np.asarray(pos_cam[f], dtype)[ids]
        E = [dtype(A * (i * SUB + 128) + B * (j * SUB + 128) + C) for A, B, C in (edge(x, y, k) for k in range(3))]
        w = np.array([E[k] / p[k, 2] for k in range(3)], dtype)
        w = w / w.sum()
        at = w @ p
        n = (w @ np.asarray(normals[f], dtype)[ids]) if normals is not None else np.cross(p[1] - p[0], p[2] - p[0])
        ln = np.sqrt((n * n).sum())
        I = dtype(ambient)
        if ln > 0:
            n = n / ln * (-1.0 if n @ at > 0 else 1.0)
            facing[f, j, i] = abs(float(n @ at)) / float(np.sqrt(at @ at))
            for l in lights:
                I = I + l[3] * max(dtype(0), -(n @ l[:3]))
        rgb[f, j, i] = to_byte(np.asarray(base, dtype) * I)
    return facing


def shade_points(rgb, prim_id, prim_base, P, base):
    rgb[(prim_id >= prim_base) & (prim_id < prim_base + P)] = to_byte(np.asarray(base, np.float64))


def fill(rgb, prim_id, bg):
    rgb[prim_id == -1] = to_byte(np.asarray(bg, np.float64))


# ---- scenes shared by the CPU and GPU tests ---------------------------------------------------------------------------------------
def uv_sphere(rings=10, segs=16, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """closed UV sphere: 2 + rings * segs vertices, outward triangles"""
    v = [(0.0, 0.0, -radius)]
    for r in range(rings):
        th = np.pi * (r + 1) / (rings + 1)
        for s in range(segs):
            ph = 2 * np.pi * s / segs
            v.append((radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), -radius * np.cos(th)))
    v.append((0.0, 0.0, radius))
    ring = lambda r, s: 1 + r * segs + s % segs  # noqa: E731
    top = len(v) - 1
    f = [(0, ring(0, s + 1), ring(0, s)) for s in range(segs)]
    for r in range(rings - 1):
        for s in range(segs):
            a, b, c, d = ring(r, s), ring(r, s + 1), ring(r + 1, s), ring(r + 1, s + 1)
            f += [(a, b, d), (a, d, c)]
    f += [(top, ring(rings - 1, s), ring(rings - 1, s + 1)) for s in range(segs)]
    return np.array(v, np.float64) + np.asarray(centre, np.float64), np.array(f, np.int32)


def camera(W, H, fov_deg=50.0, near=0.05, view=None):
    f = 0.5 * min(W, H) / np.tan(np.radians(fov_deg) / 2)
    return dict(view=np.eye(3, 4) if view is None else np.asarray(view, np.float64), fx=f, fy=f, cx=W / 2, cy=H / 2, near=near)


def quad_scene():
    """a fronto-parallel quad of two triangles at z = 2 whose image is the pixel rectangle [5.5, 20.5] x [3.5, 12.5] at 32 x 24, f = 16:
    corners ON pixel centres, so the tie rule decides the border, and the diagonal passes through centres"""
    W, H, f, z = 32, 24, 16.0, 2.0
    cam = dict(view=np.eye(3, 4), fx=f, fy=f, cx=16.0, cy=12.0, near=0.1)
    cx = lambda u: (u - 16.0) * z / f  # noqa: E731
    cy = lambda v: (v - 12.0) * z / f  # noqa: E731
    verts = np.array([[cx(5.5), cy(3.5), z], [cx(20.5), cy(3.5), z], [cx(20.5), cy(12.5), z], [cx(5.5), cy(12.5), z]])
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    # the tie rule (A > 0, or A == 0 and B < 0) with y pointing down: the left edge (A > 0) and the bottom edge (A == 0, B < 0) own their
    # centres - columns 5.5 in, 20.5 out; rows 12.5 in, 3.5 out (the "top-left" rule of a y-up frame)
    expect = np.zeros((H, W), bool)
    expect[4:13, 5:20] = True
    return dict(W=W, H=H, cam=cam, verts=verts, faces=faces, expect=expect)


def soup_scene(seed=3, n=64, W=48, H=40):
    """random triangles of both windings in front of the camera, some reaching outside the image, plus degenerate ones (a repeated
    vertex, three collinear vertices) and one with a vertex behind the near plane"""
    rng = np.random.default_rng(seed)
    cam = camera(W, H)
    centres = rng.uniform([-1.2, -1.0, 2.0], [1.2, 1.0, 4.0], size=(n, 3))
    verts = (centres[:, None, :] + rng.normal(size=(n, 3, 3)) * [0.35, 0.35, 0.2]).reshape(-1, 3)
    faces = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    faces[5] = [15, 15, 16]  # a repeated vertex
    verts[3 * 9: 3 * 9 + 3] = [[0.0, 0.0, 3.0], [0.5, 0.5, 3.0], [1.0, 1.0, 3.0]]  # collinear
    verts[3 * 12, 2] = -1.0  # behind the camera: the triangle is dropped whole
    return dict(W=W, H=H, cam=cam, verts=verts, faces=faces)
