"""The scenes of the renderer's tests, and their float64 restatement, computed once per process and shared (never modified):
  quad          the fronto-parallel quad of render_restatement.quad_scene, 32 x 24
  soup          64 random triangles of both windings with degenerate ones, 48 x 40 (no multiple of the 16-pixel tile)
  hand_spheres  a MANO-shaped hand (tests/mano_fixture.py) with per-frame vertices and two intersecting UV spheres with per-frame poses,
                96 x 80, 3 frames
  points1 / points5   500 points as splats of 1 and 5 pixels, 48 x 40
A scene: W, H, F, cam, items [kind, verts (V,3) | (F,V,3), faces | None, model (F,3,4) | None, point_size]."""
import numpy as np

import mano_fixture
import render_restatement as R

NAMES = ["quad", "soup", "hand_spheres", "points1", "points5"]
_cache = {}


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _poses(F, axis, step, shift):
    m = np.zeros((F, 3, 4))
    for f in range(F):
        m[f, :, :3] = _rot(axis, step * f)
        m[f, :, 3] = np.asarray(shift) * f
    return m


def scene(name):
    if name == "quad":
        q = R.quad_scene()
        return dict(W=q["W"], H=q["H"], F=1, cam=q["cam"], items=[dict(kind="mesh", verts=q["verts"], faces=q["faces"], model=None)])
    if name == "soup":
        s = R.soup_scene()
        return dict(W=s["W"], H=s["H"], F=1, cam=s["cam"], items=[dict(kind="mesh", verts=s["verts"], faces=s["faces"], model=None)])
    if name == "hand_spheres":
        F, W, H = 3, 96, 80
        arr = mano_fixture.synthetic_arrays(778)
        rng = np.random.default_rng(11)
        hand = arr["v_template"][None] + np.arange(F)[:, None, None] * np.array([0.004, -0.002, 0.003]) + rng.normal(size=(F, 778, 3)) * 2e-4
        s1, f1 = R.uv_sphere(10, 16, 0.045, (0.10, 0.01, 0.02))
        s2, f2 = R.uv_sphere(10, 16, 0.040, (0.14, 0.00, 0.04))  # intersects the first
        view = np.concatenate([_rot((1.0, 0.3, 0.0), 0.4), [[-0.10], [0.0], [0.45]]], axis=1)
        return dict(W=W, H=H, F=F, cam=R.camera(W, H, fov_deg=35.0, near=0.05, view=view),
                    items=[dict(kind="mesh", verts=hand, faces=arr["faces"].astype(np.int32), model=None),
                           dict(kind="mesh", verts=s1, faces=f1, model=_poses(F, (0.2, 1.0, 0.1), 0.3, (0.003, 0.0, -0.002))),
                           dict(kind="mesh", verts=s2, faces=f2, model=_poses(F, (1.0, 0.0, 0.5), -0.2, (-0.004, 0.002, 0.0)))])
    if name in ("points1", "points5"):
        W, H = 48, 40
        rng = np.random.default_rng(21)
        pts = rng.uniform([-1.6, -1.3, 1.5], [1.6, 1.3, 4.0], size=(500, 3))  # some fall outside the image
        pts[7, 2] = -0.5  # behind the camera
        return dict(W=W, H=H, F=1, cam=R.camera(W, H), items=[dict(kind="points", verts=pts, faces=None, model=None, point_size=int(name[-1]))])
    raise KeyError(name)


def counts(sc):
    return [int(it["faces"].shape[0]) if it["kind"] == "mesh" else int(it["verts"].shape[-2]) for it in sc["items"]]


def bases(sc):
    return [int(b) for b in np.concatenate([[0], np.cumsum(counts(sc))[:-1]])]


def draw(sc, proj, dtype=np.float64):
    """the items of `sc` rasterised in order from their projections proj = [(pos_cam, xy)] -> Buffers"""
    buf = R.Buffers(sc["F"], sc["H"], sc["W"], dtype)
    for it, (pos, xy), base in zip(sc["items"], proj, bases(sc)):
        if it["kind"] == "mesh":
            R.raster(buf, xy, pos, it["faces"], base)
        else:
            R.points(buf, xy, pos, it["point_size"], base)
    return buf


def project_items(sc, dtype=np.float64):
    c = sc["cam"]
    return [R.project(it["verts"], it["model"], c["view"], c["fx"], c["fy"], c["cx"], c["cy"], c["near"], F=sc["F"], dtype=dtype) for it in sc["items"]]


def reference(name):
    """the scene and its float64 restatement from the restatement's own projection: dict(scene, proj [(pos, xy, uv)], buf)"""
    if name not in _cache:
        sc = scene(name)
        proj = project_items(sc)
        _cache[name] = dict(scene=sc, proj=proj, buf=draw(sc, [(p, xy) for p, xy, _ in proj]))
    return _cache[name]


def vertex_normals(verts, faces):
    """unit area-weighted vertex normals of (F, V, 3) float64 vertices"""
    v = np.asarray(verts, np.float64)
    n = np.zeros_like(v)
    fn = np.cross(v[:, faces[:, 1]] - v[:, faces[:, 0]], v[:, faces[:, 2]] - v[:, faces[:, 0]])
    for k in range(3):
        for f in range(v.shape[0]):
            np.add.at(n[f], faces[:, k], fn[f])
    return n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-30)
