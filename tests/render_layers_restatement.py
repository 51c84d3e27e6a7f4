"""The renderer's second step (include/tamf_render.h: depth peeling, per-vertex colours, composite, resolve) restated in numpy, on top
of tests/render_restatement.py, whose coverage and depth rules it reuses unchanged: per pixel EVERY candidate (depth, id) is collected,
sorted by (depth, id), and layer k is the k-th of them.  Real arithmetic is float64 unless a dtype is given.  No torch, no GPU.
The scenes the layer tests add are here too: `shells`, `points_mesh`."""
import numpy as np

import render_restatement as R
import render_scenes as S

NAMES = ["hand_spheres", "soup", "shells", "points_mesh"]  # the scenes of the peeling tests
K = 4  # the layers they peel
_cache = {}


class Collector:
    """stands where R.Buffers stands in R.raster / R.points: keeps every candidate instead of the nearest"""

    def __init__(self, F, H, W, dtype=np.float64):
        self.dtype = dtype
        self.depth = np.empty((F, H, W), dtype)  # (its shape is what the rasterisers read)
        self.pix, self.d, self.pid = [], [], []

    def offer(self, f, ys, xs, d, pid):
        F, H, W = self.depth.shape
        flat = (f * H + np.asarray(ys, np.int64)) * W + np.asarray(xs, np.int64)
        self.pix.append(flat.ravel())
        self.d.append(np.broadcast_to(np.asarray(d, self.dtype), flat.shape).ravel())
        self.pid.append(np.full(flat.size, pid, np.int64))


def collect(sc, proj, dtype=np.float64):
    """every candidate of the scene's items, drawn in order from proj = [(pos_cam, xy)] -> Collector"""
    col = Collector(sc["F"], sc["H"], sc["W"], dtype)
    for it, (pos, xy), base in zip(sc["items"], proj, S.bases(sc)):
        if it["kind"] == "mesh":
            R.raster(col, xy, pos, it["faces"], base)
        else:
            R.points(col, xy, pos, it["point_size"], base)
    return col


class Layers:
    """depth (K,F,H,W) with +inf where a layer is empty, prim_id (K,F,H,W) with -1 there, count (F,H,W) candidates per pixel, and
    near_tie (F,H,W): an adjacent pair among the pixel's first K + 1 sorted candidates lies within `tol` relative depth"""

    def __init__(self, col, K, tol=R.NEAR_TIE):
        shape = col.depth.shape
        n = int(np.prod(shape))
        self.depth = np.full((K, n), np.inf, col.dtype)
        self.prim_id = np.full((K, n), -1, np.int64)
        self.near_tie = np.zeros(n, bool)
        self.count = np.zeros(n, np.int64)
        if col.pix:
            pix, d, pid = np.concatenate(col.pix), np.concatenate(col.d), np.concatenate(col.pid)
            order = np.lexsort((pid, d, pix))
            pix, d, pid = pix[order], d[order], pid[order]
            first = np.r_[True, pix[1:] != pix[:-1]]
            start = np.maximum.accumulate(np.where(first, np.arange(pix.size), 0))
            rank = np.arange(pix.size) - start
            np.add.at(self.count, pix, 1)
            keep = rank < K
            self.depth[rank[keep], pix[keep]] = d[keep]
            self.prim_id[rank[keep], pix[keep]] = pid[keep]
            pair = ~first & (rank <= K)  # candidate `rank` against the one before it: both among the first K + 1
            close = np.zeros(pix.size, bool)
            close[1:] = (d[1:] - d[:-1]) <= tol * np.abs(d[1:])
            self.near_tie[pix[pair & close]] = True
        self.depth, self.prim_id = self.depth.reshape((K,) + shape), self.prim_id.reshape((K,) + shape)
        self.near_tie, self.count = self.near_tie.reshape(shape), self.count.reshape(shape)

    def near_tie_share(self):
        covered = int((self.count > 0).sum())
        return (int(self.near_tie.sum()) / covered) if covered else 0.0


# ---- colours, composite, resolve --------------------------------------------------------------------------------------------------
def shade_mesh_colors(rgb, prim_id, xy, pos_cam, normals, faces, prim_base, colors, ambient, lights, dtype=np.float64):
    """R.shade_mesh with the base colour sum_k w_k c_k of colors (V,3) or (F,V,3), blended by the weights of the normals"""
    faces, colors = np.asarray(faces), np.asarray(colors, dtype)
    lights = np.asarray(lights, dtype).reshape(-1, 4)
    for f, j, i in zip(*np.nonzero((prim_id >= prim_base) & (prim_id < prim_base + faces.shape[0]))):
        o = R.oriented(xy[f], faces[prim_id[f, j, i] - prim_base])
        if o is None:
            continue
        x, y, ids, a2 = o
        p = np.asarray(pos_cam[f], dtype)[ids]
        E = [dtype(A * (i * R.SUB + 128) + B * (j * R.SUB + 128) + C) for A, B, C in (R.edge(x, y, k) for k in range(3))]
        w = np.array([E[k] / p[k, 2] for k in range(3)], dtype)
        w = w / w.sum()
        at = w @ p
        n = (w @ np.asarray(normals[f], dtype)[ids]) if normals is not None else np.cross(p[1] - p[0], p[2] - p[0])
        ln = np.sqrt((n * n).sum())
        I = dtype(ambient)
        if ln > 0:
            n = n / ln * (-1.0 if n @ at > 0 else 1.0)
            for l in lights:
                I = I + l[3] * max(dtype(0), -(n @ l[:3]))
        base = w @ (colors[f] if colors.ndim == 3 else colors)[ids]
        rgb[f, j, i] = R.to_byte(base * I)


def shade_points_colors(rgb, prim_id, prim_base, colors):
    colors = np.asarray(colors, np.float64)
    P = colors.shape[-2]
    for f, j, i in zip(*np.nonzero((prim_id >= prim_base) & (prim_id < prim_base + P))):
        rgb[f, j, i] = R.to_byte((colors[f] if colors.ndim == 3 else colors)[prim_id[f, j, i] - prim_base])


def composite(layer_rgb, layer_id, bases, counts, alphas, bg):
    """layer_rgb (K,F,H,W,3) uint8, layer_id (K,F,H,W) -> (the image (F,H,W,3) uint8, the float64 colour before the byte rule)"""
    Kk = layer_id.shape[0]
    C = np.broadcast_to(np.clip(np.asarray(bg, np.float64), 0.0, 1.0), layer_id.shape[1:] + (3,)).copy()
    for k in range(Kk - 1, -1, -1):
        for b, n, a in zip(bases, counts, alphas):
            m = (layer_id[k] >= b) & (layer_id[k] < b + n)
            C[m] = float(a) * (layer_rgb[k][m].astype(np.float64) / 255.0) + (1.0 - float(a)) * C[m]
    return R.to_byte(C), C


def resolve(rgb, s):
    """(F, s H, s W, 3) uint8 -> (F, H, W, 3): (sum of the s * s bytes + s * s / 2) / (s * s) in integers"""
    F, Hs, Ws, _ = rgb.shape
    blocks = rgb.astype(np.int64).reshape(F, Hs // s, s, Ws // s, s, 3).sum(axis=(2, 4))
    return ((blocks + (s * s) // 2) // (s * s)).astype(np.uint8)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def scene(name):
    """`shells`: three items, each a pair of sphere shells around one centre, the radii interleaved between the items (0.50 / 0.26,
    0.42 / 0.18, 0.34 / 0.10): a ray through the middle meets twelve fragments that alternate between the three calls, 50 x 44.
    `points_mesh`: a sphere between two sheets of points (splats of 3 pixels) and a second cloud inside it, 40 x 36.
    Neither size is a multiple of the 16-pixel tile.  The other names are those of tests/render_scenes.py."""
    if name == "shells":
        W, H = 50, 44
        items = []
        for k, (r_out, r_in) in enumerate(((0.50, 0.26), (0.42, 0.18), (0.34, 0.10))):
            centre = (0.03 * k - 0.02, 0.015 * k, 3.0 + 0.01 * k)
            a, fa = R.uv_sphere(7 + k, 11 + 2 * k, r_out, centre)
            b, fb = R.uv_sphere(5 + k, 9 + k, r_in, centre)
            items.append(dict(kind="mesh", verts=np.concatenate([a, b]), faces=np.concatenate([fa, fb + a.shape[0]]).astype(np.int32), model=None))
        return dict(W=W, H=H, F=1, cam=R.camera(W, H, fov_deg=24.0), items=items)
    if name == "points_mesh":
        W, H = 40, 36
        rng = np.random.default_rng(5)
        v, f = R.uv_sphere(8, 12, 0.6, (0.05, -0.03, 3.0))
        sheet = rng.uniform([-1.0, -0.9, 2.0], [1.0, 0.9, 4.0], size=(260, 3))
        inner = rng.normal(size=(120, 3)) * 0.2 + [0.05, -0.03, 3.0]
        return dict(W=W, H=H, F=1, cam=R.camera(W, H, fov_deg=40.0),
                    items=[dict(kind="points", verts=sheet, faces=None, model=None, point_size=3), dict(kind="mesh", verts=v, faces=f, model=None),
                           dict(kind="points", verts=inner, faces=None, model=None, point_size=3)])
    return S.scene(name)


def reference(name, layers=K):
    """the scene and its float64 restatement from the restatement's own projection, computed once: dict(scene, proj, layers)"""
    if name not in _cache:
        sc = scene(name)
        proj = S.project_items(sc)
        _cache[name] = dict(scene=sc, proj=proj, layers=Layers(collect(sc, [(p, xy) for p, xy, _ in proj]), layers))
    return _cache[name]


def vertex_palette(n, seed, frames=None):
    """deterministic colours in [0, 1]: (n, 3), or (frames, n, 3)"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, size=((n, 3) if frames is None else (frames, n, 3))).astype(np.float32)
