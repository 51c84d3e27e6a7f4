"""Offscreen rendering of hand / object clips on the GPU (libtamf_render.so, include/tamf_render.h): stands where the reference's
viewers (script/viz_seg.py, script/debug/debug_*_sample.py) and dev_fn/util/vis_pyrender_util.py:PyMultiObjRenderer need Open3D or
pyrender with OpenGL and a display.

HipRenderer      meshes and point clouds with static or per-frame vertices and an optional per-frame rigid pose -> rgb, depth, prim_id;
                 per-vertex / per-point colours, see-through items (alpha, `layers` peeled depth layers), supersampling (`ssaa`)
contact_colors   hand-to-object distances -> a heat map to pass as vertex colours
look_at_camera   one fixed pinhole camera per clip, fitted in float64 to the bounding sphere of everything in it
default_lights   the arrangement of PyMultiObjRenderer._create_raymond_lights in this package's camera frame; ambient 0.2
write_png        zlib + struct only: no imaging package at run time
write_apng       the frames of a clip as one animated PNG that plays in a browser, written the same way; read_apng reads it back
contact_sheet    frames tiled into one image

The image is this package's own rasterisation and Lambert shading, NOT pyrender's PBR output: no textures, no shadows, no clipping
(a triangle with a vertex in front of the near plane is dropped, in every layer); fragments beyond the last peeled layer are
dropped; anti-aliasing is the box filter of `ssaa`.  No CPU or torch fall-back for the kernels."""
from __future__ import annotations

import ctypes
import struct
import zlib
from ctypes import c_float, c_int32, c_void_p
from typing import NamedTuple, Optional, Sequence

import numpy as np

AMBIENT = 0.2  # PyMultiObjRenderer: pyrender.Scene(ambient_light=[0.2, 0.2, 0.2])
PROJECTION_BYTES = 256 << 20  # render() chunks the frames so that the projection buffers of a chunk stay under this
MAX_SIDE, MAX_POINT_SIZE, MAX_LIGHTS = 4096, 15, 8
MAX_LAYERS, MAX_ITEMS = 8, 64  # tamf_render_composite
LAYER_BYTES = 11  # per pixel of a peeled layer: depth (4 B) + prim_id (4 B) + rgb (3 B)


class Camera(NamedTuple):
    view: np.ndarray  # (3, 4) world -> camera, OpenCV frame: x right, y down, z forward
    fx: float
    fy: float
    cx: float
    cy: float
    near: float


class CameraStruct(ctypes.Structure):  # tamf_render_camera
    _fields_ = [("view", c_float * 12), ("fx", c_float), ("fy", c_float), ("cx", c_float), ("cy", c_float), ("near", c_float)]


def camera_struct(cam: Camera) -> CameraStruct:
    view = np.asarray(cam.view, np.float64)
    if view.shape == (4, 4):
        view = view[:3]
    if view.shape != (3, 4):
        raise ValueError(f"camera view: expected (3, 4) or (4, 4), got {view.shape}")
    return CameraStruct((c_float * 12)(*[float(x) for x in view.reshape(-1)]), float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy), float(cam.near))


_bound = None


def _bind():
    global _bound
    if _bound is None:
        from . import _lib

        lib = _lib.load_render()
        P, I = c_void_p, c_int32
        lib.tamf_render_last_error.restype = ctypes.c_char_p
        lib.tamf_render_last_error.argtypes = []
        lib.tamf_render_project.argtypes = [P, P, P, I, I, I, P, P, P]
        lib.tamf_render_clear.argtypes = [P, P, I, I, I, P]
        lib.tamf_render_raster.argtypes = [P, P, P, I, I, I, I, I, I, P, P, P]
        lib.tamf_render_points.argtypes = [P, P, I, I, I, I, I, I, P, P, P]
        lib.tamf_render_shade_mesh.argtypes = [P, P, P, P, P, I, I, I, I, I, I, P, c_float, P, I, P, P]
        lib.tamf_render_shade_points.argtypes = [P, I, I, I, I, I, P, P, P]
        lib.tamf_render_fill.argtypes = [P, I, I, I, P, P, P]
        lib.tamf_render_raster_behind.argtypes = [P, P, P, I, I, I, I, I, I, P, P, P, P, P]
        lib.tamf_render_points_behind.argtypes = [P, P, I, I, I, I, I, I, P, P, P, P, P]
        lib.tamf_render_shade_mesh_colors.argtypes = [P, P, P, P, P, I, I, I, I, I, I, P, I, c_float, P, I, P, P]
        lib.tamf_render_shade_points_colors.argtypes = [P, I, I, I, I, I, P, I, P, P]
        lib.tamf_render_composite.argtypes = [P, P, I, I, I, I, P, P, P, I, P, P, P]
        lib.tamf_render_resolve.argtypes = [P, I, I, I, I, P, P]
        _bound = lib
    return _bound


def _check(lib, rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"libtamf_render: {lib.tamf_render_last_error().decode()} (status {rc})")


def _floats(values, n=None):
    a = np.ascontiguousarray(np.asarray(values, np.float32).reshape(-1))
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} values, got {a.size}")
    return a


def default_lights() -> np.ndarray:
    """(3, 4) float64 rows (unit direction the light travels, strength): three directional lights 30 degrees off the optical axis and
    120 degrees apart, shining away from the viewer - PyMultiObjRenderer._create_raymond_lights (theta = pi / 6, phi = 0, 2 pi / 3,
    4 pi / 3) carried from pyrender's OpenGL camera frame into the OpenCV one (y and z negated).  pyrender's intensity 1.0 goes
    through its BRDF's 1 / pi; here the strength is that factor, so three head-on lights and the ambient term stay below 1."""
    rows = []
    for phi in (0.0, 2.0 * np.pi / 3.0, 4.0 * np.pi / 3.0):
        theta = np.pi / 6.0
        gl = -np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)])  # the light looks along -z of its node
        rows.append([gl[0], -gl[1], -gl[2], 1.0 / np.pi])
    return np.asarray(rows, np.float64)


def look_at_camera(points, width: int, height: int, fov_deg: float = 45.0, forward=(0.0, 0.0, 1.0), up=(0.0, -1.0, 0.0), margin: float = 1.1) -> Camera:
    """One fixed camera for a clip: looks along `forward` (world frame) at the centre of the bounding sphere of `points` (any shape
    (..., 3); non-finite rows ignored) from the distance at which the sphere, enlarged by `margin`, fills the field of view `fov_deg`
    of the smaller image side.  `up` is the world direction that points up in the image.  Everything in float64."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    if p.shape[0] == 0:
        raise ValueError("look_at_camera: no finite point")
    if not 0.0 < fov_deg < 180.0:
        raise ValueError(f"fov_deg must lie in (0, 180), got {fov_deg}")
    centre = 0.5 * (p.min(axis=0) + p.max(axis=0))
    radius = max(float(np.sqrt(((p - centre) ** 2).sum(axis=1).max())), 1e-6)
    z = np.asarray(forward, np.float64)
    z = z / np.linalg.norm(z)
    x = np.cross(-np.asarray(up, np.float64), z)  # y points down: x = down x forward ... right-handed with y = z x x
    if np.linalg.norm(x) < 1e-9:
        raise ValueError("look_at_camera: `up` is parallel to `forward`")
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    half = np.radians(fov_deg) / 2.0
    dist = margin * radius / np.sin(half)
    eye = centre - dist * z
    R = np.stack([x, y, z])  # world -> camera
    view = np.concatenate([R, (-R @ eye)[:, None]], axis=1)
    f = 0.5 * min(width, height) / np.tan(half)
    return Camera(view=view, fx=f, fy=f, cx=width / 2.0, cy=height / 2.0, near=max(1e-4, 0.5 * (dist - radius)))


def tslrot6d_to_matrix(rows):
    """(F, 9) = tsl | rot6d rows (the package's object trajectories) -> (F, 3, 4) float64: metrics.siv.tslrot6d_to_transf's rotation"""
    from .metrics.siv import tslrot6d_to_transf

    return tslrot6d_to_transf(np.asarray(rows, np.float64))[..., :3, :]


def _pose(pose, name):
    """None, (F, 4, 4) / (F, 3, 4) matrices or (F, 9) tslrot6d rows -> (F, 3, 4) float64 or None"""
    if pose is None:
        return None
    a = pose.detach().cpu().numpy() if hasattr(pose, "detach") else np.asarray(pose)
    if a.ndim == 2 and a.shape[1] == 9:
        return tslrot6d_to_matrix(a)
    if a.ndim == 3 and a.shape[1:] in ((4, 4), (3, 4)):
        return np.ascontiguousarray(a[:, :3, :], np.float64)
    raise ValueError(f"{name}: pose must be (F, 4, 4), (F, 3, 4) or (F, 9) tslrot6d rows, got {a.shape}")


class _Item(NamedTuple):
    kind: str  # "mesh" | "points"
    verts: object  # torch float32 device tensor (V, 3) or (F, V, 3)
    pose: Optional[np.ndarray]  # (F, 3, 4) float64
    faces: object  # torch int32 device (Nf, 3); None for points
    faces_host: Optional[np.ndarray]
    color: np.ndarray
    smooth: bool
    point_size: int
    frames: Optional[int]  # None: static, any number of frames
    colors: object = None  # torch float32 device tensor (V, 3) or (F, V, 3), or None: `color` everywhere
    alpha: float = 1.0


class HipRenderer:
    """Collect the meshes and point clouds of a clip, then render(camera).  Primitive ids: the items in the order they were added,
    item k's primitives numbered from `prim_base[k]` (the sum of the counts before it)."""

    def __init__(self, width: int, height: int, device="cuda:0", background=(0.0, 0.0, 0.0), ambient: float = AMBIENT, lights=None):
        if not (1 <= int(width) <= MAX_SIDE and 1 <= int(height) <= MAX_SIDE):
            raise ValueError(f"width and height must lie in [1, {MAX_SIDE}], got {width} x {height}")
        self.width, self.height, self.device = int(width), int(height), device
        self.background, self.ambient = _floats(background, 3), float(ambient)
        self.lights = _floats(default_lights() if lights is None else lights).reshape(-1, 4)
        if self.lights.shape[0] > MAX_LIGHTS:
            raise ValueError(f"at most {MAX_LIGHTS} lights, got {self.lights.shape[0]}")
        self.items = []

    # -- scene ---------------------------------------------------------------------------------------------------------------
    def _verts(self, verts, pose, name):
        import torch

        from .hip_backend import require_gpu

        dev = require_gpu(self.device)
        v = torch.as_tensor(verts).detach().to(device=dev, dtype=torch.float32).contiguous()
        if v.dim() not in (2, 3) or v.shape[-1] != 3 or v.shape[-2] < 1:
            raise ValueError(f"{name}: vertices must be (V, 3) or (F, V, 3), got {tuple(v.shape)}")
        m = _pose(pose, name)
        frames = int(v.shape[0]) if v.dim() == 3 else None
        if m is not None:
            if frames is not None and frames != m.shape[0]:
                raise ValueError(f"{name}: {frames} frames of vertices but {m.shape[0]} poses")
            frames = int(m.shape[0])
        return v, m, frames

    def _colors(self, colors, alpha, v, frames, name):
        """the checks of vertex_colors / point_colors and alpha, before anything reaches the library -> (device tensor or None, frames, alpha)"""
        import torch

        alpha = float(alpha)
        if not 0.0 < alpha <= 1.0:  # (false for NaN)
            raise ValueError(f"{name}: alpha must lie in (0, 1], got {alpha}")
        if colors is None:
            return None, frames, alpha
        c = torch.as_tensor(colors).detach()
        V = int(v.shape[-2])
        if c.dim() not in (2, 3) or tuple(c.shape[-2:]) != (V, 3) or not c.dtype.is_floating_point:
            raise ValueError(f"{name}: colours must be float ({V}, 3) or (F, {V}, 3), got {tuple(c.shape)} {c.dtype}")
        if not bool(torch.isfinite(c).all()):
            raise ValueError(f"{name}: a non-finite colour")
        if c.dim() == 3:
            if frames is not None and frames != int(c.shape[0]):
                raise ValueError(f"{name}: {frames} frames of vertices or poses but {int(c.shape[0])} of colours")
            frames = int(c.shape[0])
        return c.to(device=v.device, dtype=torch.float32).contiguous(), frames, alpha

    def add_mesh(self, verts, faces, color=(0.8, 0.8, 0.8), pose=None, smooth: bool = False, name: str = "mesh", vertex_colors=None,
                 alpha: float = 1.0) -> int:
        """verts (V, 3) static or (F, V, 3) per frame; faces (Nf, 3); pose None, (F, 4, 4) / (F, 3, 4) or (F, 9) tslrot6d rows, applied
        to the vertices before the camera; smooth: shade with geometry.vertex_normals instead of face normals -> the item's index.
        vertex_colors (V, 3) or (F, V, 3), float in [0, 1]: blended over each triangle in place of `color`; alpha in (0, 1]: below 1 the
        item is see-through where render() is given enough `layers`.  The face indices are range-checked here, once."""
        import torch

        v, m, frames = self._verts(verts, pose, name)
        colors, frames, alpha = self._colors(vertex_colors, alpha, v, frames, name)
        f = np.asarray(faces.detach().cpu().numpy() if hasattr(faces, "detach") else faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
            raise ValueError(f"{name}: faces must be (Nf, 3) with Nf >= 1, got {f.shape}")
        V = int(v.shape[-2])
        if int(f.min()) < 0 or int(f.max()) >= V:
            raise ValueError(f"{name}: face indices outside [0, {V}) (min {int(f.min())}, max {int(f.max())})")
        f32 = np.ascontiguousarray(f, np.int32)
        self.items.append(_Item("mesh", v, m, torch.from_numpy(f32).to(v.device), f32, _floats(color, 3), bool(smooth), 0, frames, colors, alpha))
        return len(self.items) - 1

    def add_points(self, points, color=(0.8, 0.8, 0.8), pose=None, point_size: int = 3, name: str = "points", point_colors=None,
                   alpha: float = 1.0) -> int:
        """points (P, 3) or (F, P, 3); each is drawn as an unlit square of point_size (odd, 1 .. 15) pixels -> the item's index.
        point_colors (P, 3) or (F, P, 3), float in [0, 1]: every splat in its own point's colour; alpha as for add_mesh"""
        if point_size % 2 != 1 or not 1 <= point_size <= MAX_POINT_SIZE:
            raise ValueError(f"{name}: point_size must be odd and lie in [1, {MAX_POINT_SIZE}], got {point_size}")
        v, m, frames = self._verts(points, pose, name)
        colors, frames, alpha = self._colors(point_colors, alpha, v, frames, name)
        self.items.append(_Item("points", v, m, None, None, _floats(color, 3), False, int(point_size), frames, colors, alpha))
        return len(self.items) - 1

    def clear_scene(self) -> None:
        self.items = []

    @property
    def counts(self):
        return [int(it.faces.shape[0]) if it.kind == "mesh" else int(it.verts.shape[-2]) for it in self.items]

    @property
    def prim_base(self):
        return [int(b) for b in np.concatenate([[0], np.cumsum(self.counts)[:-1]])] if self.items else []

    def n_frames(self) -> int:
        frames = {it.frames for it in self.items if it.frames is not None}
        if len(frames) > 1:
            raise ValueError(f"the items disagree on the number of frames: {sorted(frames)}")
        return frames.pop() if frames else 1

    def frames_per_chunk(self, layers: int = 1, ssaa: int = 1) -> int:
        """frames rendered per pass: xy (8 B) + pos_cam (12 B) per vertex and frame, + 12 B of normals for smooth meshes; on the layered
        path also the `layers` peeled layers of ssaa^2 * width * height pixels (depth, prim_id and rgb: 11 B each) and the composited
        image (3 B a pixel)"""
        per_frame = sum(int(it.verts.shape[-2]) * (32 if it.smooth else 20) for it in self.items)
        pixels = ssaa * ssaa * self.width * self.height
        if not self._plain(layers, ssaa):
            per_frame += pixels * (layers * LAYER_BYTES + 3)
        return max(1, min(65535, PROJECTION_BYTES // max(1, per_frame), (2 ** 31 - 1) // pixels))

    def _plain(self, layers: int, ssaa: int) -> bool:
        """one opaque layer at the image's own size: drawn straight into the outputs, without a composite"""
        return layers == 1 and ssaa == 1 and all(it.alpha == 1.0 for it in self.items)

    # -- render --------------------------------------------------------------------------------------------------------------
    def render(self, camera: Camera, frames: Optional[Sequence[int]] = None, layers: int = 1, ssaa: int = 1):
        """-> (rgb (F, H, W, 3) uint8, depth (F, H, W) float32 with +inf where nothing was drawn, prim_id (F, H, W) int32 with -1 there)
        device tensors; `frames`: the frame indices to render (default: all).
        layers = K in 1 .. 8: the K nearest fragments of every pixel are peeled (layer 0 by the plain calls, layer k by the _behind calls
        over all items with layer k - 1 as floor), each layer is shaded, and the layers are composited back to front with the items'
        alphas; fragments beyond layer K - 1 are dropped.  ssaa = s in 1 .. 4: everything is drawn at (s H, s W) with the intrinsics scaled
        by s and the splats at s * point_size pixels (+ 1 when that is even), and s x s blocks are averaged.
        rgb is the final image.  depth and prim_id are LAYER 0's, the nearest fragment whatever its alpha; with ssaa > 1 they are taken
        at the top-left sub-sample of each pixel.  layers = 1, ssaa = 1 with every alpha 1 is the plain path, call for call."""
        import torch

        from .hip_backend import _stream_ptr, require_gpu

        if not self.items:
            raise ValueError("nothing to render: add a mesh or a point cloud first")
        if sum(self.counts) > 2 ** 31 - 1:
            raise ValueError("more than 2^31 - 1 primitives")
        layers, ssaa = int(layers), int(ssaa)
        if not 1 <= layers <= MAX_LAYERS:
            raise ValueError(f"layers must lie in [1, {MAX_LAYERS}], got {layers}")
        if not 1 <= ssaa <= 4:
            raise ValueError(f"ssaa must lie in [1, 4], got {ssaa}")
        if ssaa * max(self.width, self.height) > MAX_SIDE:
            raise ValueError(f"ssaa * width and ssaa * height must not exceed {MAX_SIDE}, got {ssaa} * ({self.width} x {self.height})")
        if not self._plain(layers, ssaa) and len(self.items) > MAX_ITEMS:
            raise ValueError(f"at most {MAX_ITEMS} items on the layered path, got {len(self.items)}")
        for it in self.items:
            if it.kind == "points" and _scaled_point_size(it.point_size, ssaa) > MAX_POINT_SIZE:
                raise ValueError(f"point_size {it.point_size} at ssaa {ssaa} is a splat of {_scaled_point_size(it.point_size, ssaa)} pixels, above {MAX_POINT_SIZE}")
        dev = require_gpu(self.device)
        total = self.n_frames()
        sel = list(range(total)) if frames is None else [int(i) for i in frames]
        if any(not 0 <= i < total for i in sel):
            raise ValueError(f"frame index outside [0, {total})")
        H, W = self.height, self.width
        rgb = torch.empty((len(sel), H, W, 3), dtype=torch.uint8, device=dev)
        depth = torch.empty((len(sel), H, W), dtype=torch.float32, device=dev)
        prim = torch.empty((len(sel), H, W), dtype=torch.int32, device=dev)
        step = self.frames_per_chunk(layers, ssaa)
        for s in range(0, len(sel), step):
            part = sel[s: s + step]
            self._render_chunk(camera, part, rgb[s: s + len(part)], depth[s: s + len(part)], prim[s: s + len(part)], dev, _stream_ptr(dev), layers, ssaa)
        return rgb, depth, prim

    def _render_chunk(self, camera, part, rgb, depth, prim, dev, stream, layers=1, ssaa=1):
        import torch

        lib = _bind()
        plain = self._plain(layers, ssaa)
        F, H, W = len(part), self.height * ssaa, self.width * ssaa
        if ssaa > 1:
            camera = camera._replace(fx=camera.fx * ssaa, fy=camera.fy * ssaa, cx=camera.cx * ssaa, cy=camera.cy * ssaa)
        cam = camera_struct(camera)
        idx = torch.as_tensor(part, dtype=torch.long, device=dev)
        P = lambda t: None if t is None else c_void_p(t.data_ptr())  # noqa: E731
        H_ = lambda a: a.ctypes.data_as(c_void_p)  # noqa: E731
        out_rgb, out_depth, out_prim = rgb, depth, prim
        if not plain:  # layer k of everything that follows: depth[k], prim[k], rgb[k]
            depth = torch.empty((layers, F, H, W), dtype=torch.float32, device=dev)
            prim = torch.empty((layers, F, H, W), dtype=torch.int32, device=dev)
            rgb = torch.empty((layers, F, H, W, 3), dtype=torch.uint8, device=dev)
        else:
            depth, prim, rgb = depth[None], prim[None], rgb[None]
        with torch.cuda.device(dev):
            self._draw_layers(lib, cam, camera, idx, part, F, H, W, layers, ssaa, depth, prim, rgb, dev, stream, P, H_)
            if plain:
                _check(lib, lib.tamf_render_fill(P(prim[0]), F, H, W, H_(self.background), P(rgb[0]), stream))
                return
            table = [np.ascontiguousarray(self.prim_base, np.int32), np.ascontiguousarray(self.counts, np.int32),
                     np.ascontiguousarray([it.alpha for it in self.items], np.float32)]
            big = out_rgb if ssaa == 1 else torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
            _check(lib, lib.tamf_render_composite(P(rgb), P(prim), layers, F, H, W, H_(table[0]), H_(table[1]), H_(table[2]), len(self.items),
                                                  H_(self.background), P(big), stream))
            if ssaa > 1:
                _check(lib, lib.tamf_render_resolve(P(big), F, self.height, self.width, ssaa, P(out_rgb), stream))
            out_depth.copy_(depth[0][:, ::ssaa, ::ssaa])
            out_prim.copy_(prim[0][:, ::ssaa, ::ssaa])

    def _draw_layers(self, lib, cam, camera, idx, part, F, H, W, layers, ssaa, depth, prim, rgb, dev, stream, P, H_):
        """layer 0 by the plain calls, layer k by the _behind calls over all items in ascending prim_base, then every layer shaded"""
        import torch

        _check(lib, lib.tamf_render_clear(P(depth[0]), P(prim[0]), F, H, W, stream))
        staged = []
        for it, base in zip(self.items, self.prim_base):
            per_frame = it.verts.dim() == 3
            v = it.verts.index_select(0, idx).contiguous() if per_frame else it.verts
            V = int(v.shape[-2])
            model = None if it.pose is None else torch.from_numpy(np.ascontiguousarray(it.pose[part], np.float32)).to(dev)
            pos = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
            xy = torch.empty((F, V, 2), dtype=torch.int32, device=dev)
            _check(lib, lib.tamf_render_project(P(v), P(model), ctypes.addressof(cam), F, V, int(per_frame), P(pos), P(xy), stream))
            size = _scaled_point_size(it.point_size, ssaa)
            if it.kind == "mesh":
                _check(lib, lib.tamf_render_raster(P(xy), P(pos), P(it.faces), F, V, int(it.faces.shape[0]), H, W, base, P(depth[0]), P(prim[0]), stream))
            else:
                _check(lib, lib.tamf_render_points(P(xy), P(pos), F, V, H, W, size, base, P(depth[0]), P(prim[0]), stream))
            staged.append((it, base, v, model, pos, xy, size))
        for k in range(1, layers):
            _check(lib, lib.tamf_render_clear(P(depth[k]), P(prim[k]), F, H, W, stream))
            for it, base, v, model, pos, xy, size in staged:
                V = int(v.shape[-2])
                if it.kind == "mesh":
                    _check(lib, lib.tamf_render_raster_behind(P(xy), P(pos), P(it.faces), F, V, int(it.faces.shape[0]), H, W, base, P(depth[k - 1]),
                                                              P(prim[k - 1]), P(depth[k]), P(prim[k]), stream))
                else:
                    _check(lib, lib.tamf_render_points_behind(P(xy), P(pos), F, V, H, W, size, base, P(depth[k - 1]), P(prim[k - 1]), P(depth[k]),
                                                              P(prim[k]), stream))
        for it, base, v, model, pos, xy, size in staged:
            V = int(v.shape[-2])
            colors = it.colors if it.colors is None or it.colors.dim() == 2 else it.colors.index_select(0, idx).contiguous()
            per_frame = int(colors is not None and colors.dim() == 3)
            normals = self._camera_normals(it, v, model, camera, F, dev) if it.kind == "mesh" and it.smooth else None
            for k in range(layers):
                if it.kind == "mesh" and colors is None:
                    _check(lib, lib.tamf_render_shade_mesh(P(prim[k]), P(xy), P(pos), P(normals), P(it.faces), F, V, int(it.faces.shape[0]), H, W,
                                                           base, H_(it.color), self.ambient, H_(self.lights), int(self.lights.shape[0]), P(rgb[k]), stream))
                elif it.kind == "mesh":
                    _check(lib, lib.tamf_render_shade_mesh_colors(P(prim[k]), P(xy), P(pos), P(normals), P(it.faces), F, V, int(it.faces.shape[0]), H, W,
                                                                  base, P(colors), per_frame, self.ambient, H_(self.lights), int(self.lights.shape[0]),
                                                                  P(rgb[k]), stream))
                elif colors is None:
                    _check(lib, lib.tamf_render_shade_points(P(prim[k]), F, H, W, base, V, H_(it.color), P(rgb[k]), stream))
                else:
                    _check(lib, lib.tamf_render_shade_points_colors(P(prim[k]), F, H, W, base, V, P(colors), per_frame, P(rgb[k]), stream))

    @staticmethod
    def _camera_normals(it, v, model, camera, F, dev):
        """unit vertex normals (geometry.vertex_normals, in the frame the vertices are given in) rotated into the camera frame: (F, V, 3)"""
        import torch

        from .geometry import vertex_normals

        n = vertex_normals(v, it.faces_host)
        if n.dim() == 2:
            n = n.unsqueeze(0).expand(F, -1, -1)
        view = np.asarray(camera.view, np.float64)[:3, :3]
        rot = view[None] if model is None else view[None] @ model[:, :, :3].double().cpu().numpy()
        rot = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(rot, (F, 3, 3)), np.float32)).to(dev)
        return torch.einsum("fij,fvj->fvi", rot, n).contiguous()


def _scaled_point_size(size: int, ssaa: int) -> int:
    """a splat of `size` pixels at `ssaa` sub-samples a side: ssaa * size, made odd"""
    s = int(size) * int(ssaa)
    return s if ssaa == 1 or s % 2 == 1 else s + 1


def contact_colors(dist, base, hot=(1.0, 0.1, 0.05), near: float = 0.005, far: float = 0.03):
    """distances (...) in metres (contact.merged_h2o_dist: hand vertex to the nearest object point; a tensor stays on its device, anything
    else goes through numpy) -> colours (..., 3) float32: w = clamp((far - d) / (far - near), 0, 1), colour = base + w * (hot - base),
    evaluated as (1 - w) * base + w * hot so that it is exactly `hot` at d <= near and exactly `base` at d >= far.  near = 5 mm is the contact threshold of the CR score; far is a display default, not a
    measurement."""
    if not float(far) > float(near):
        raise ValueError(f"contact_colors: far must exceed near, got near = {near}, far = {far}")
    if hasattr(dist, "detach"):
        import torch

        d = dist.detach().to(torch.float32)
        b, h = (torch.tensor([float(x) for x in c], dtype=torch.float32, device=d.device) for c in (base, hot))
        w = ((float(far) - d) / (float(far) - float(near))).clamp(0.0, 1.0)
        return (1.0 - w)[..., None] * b + w[..., None] * h
    d = np.asarray(dist, np.float32)
    b, h = _floats(base, 3), _floats(hot, 3)
    w = np.clip((np.float32(far) - d) / np.float32(float(far) - float(near)), 0.0, 1.0).astype(np.float32)
    return (np.float32(1.0) - w)[..., None] * b + w[..., None] * h


def penetration_colors(depth, inside, base, hot=(0.55, 0.10, 0.85), far: float = 0.01):
    """depths (...) in metres and inside (...) bool (meshdist.MeshSet.distance: distance of a hand vertex to an object's mesh, and
    whether it lies inside it; tensors stay on their device, anything else goes through numpy) -> colours (..., 3) float32:
    w = clamp(depth / far, 0, 1) where inside, 0 elsewhere; colour = (1 - w) * base + w * hot: exactly `base` outside and at depth 0,
    exactly `hot` at depth >= far.  far is a display default, not a measurement."""
    if not float(far) > 0.0:
        raise ValueError(f"penetration_colors: far must be positive, got {far}")
    if hasattr(depth, "detach"):
        import torch

        d = depth.detach().to(torch.float32)
        m = torch.as_tensor(inside, device=d.device).to(torch.bool)
        b, h = (torch.tensor([float(x) for x in c], dtype=torch.float32, device=d.device) for c in (base, hot))
        w = torch.where(m, (d / float(far)).clamp(0.0, 1.0), torch.zeros_like(d))
        return (1.0 - w)[..., None] * b + w[..., None] * h
    d = np.asarray(depth, np.float32)
    b, h = _floats(base, 3), _floats(hot, 3)
    w = np.where(np.asarray(inside, bool), np.clip(d / np.float32(far), 0.0, 1.0), 0.0).astype(np.float32)
    return (np.float32(1.0) - w)[..., None] * b + w[..., None] * h


# ---- images ---------------------------------------------------------------------------------------------------------------------
def _png_chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def _png_rows(a: np.ndarray) -> bytes:
    """(H, W, 3) uint8 -> the deflated scanlines, filter 0 per row"""
    h, w = a.shape[:2]
    return zlib.compress(np.concatenate([np.zeros((h, 1), np.uint8), np.ascontiguousarray(a).reshape(h, w * 3)], axis=1).tobytes(), 6)


def write_png(path: str, rgb) -> None:
    """(H, W, 3) uint8 (numpy or tensor) -> an 8-bit RGB PNG, written with zlib and struct only"""
    a = rgb.detach().cpu().numpy() if hasattr(rgb, "detach") else np.asarray(rgb)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: expected (H, W, 3) uint8, got {a.shape} {a.dtype}")
    h, w = a.shape[:2]
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + _png_chunk(b"IDAT", _png_rows(a)) + _png_chunk(b"IEND", b""))


def read_png(path: str) -> np.ndarray:
    """what write_png wrote -> (H, W, 3) uint8 (8-bit RGB, filter 0 only: not a general decoder)"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG")
    pos, idat, size = 8, b"", None
    while pos < len(data):
        (n,), tag = struct.unpack(">I", data[pos: pos + 4]), data[pos + 4: pos + 8]
        body = data[pos + 8: pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n: pos + 12 + n])[0] != (zlib.crc32(tag + body) & 0xFFFFFFFF):
            raise ValueError(f"{path}: bad CRC in chunk {tag!r}")
        if tag == b"IHDR":
            w, h, bits, kind, _, _, interlace = struct.unpack(">IIBBBBB", body)
            if (bits, kind, interlace) != (8, 2, 0):
                raise ValueError(f"{path}: not an 8-bit RGB non-interlaced PNG")
            size = (h, w)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    h, w = size
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    if rows[:, 0].any():
        raise ValueError(f"{path}: filtered rows (not written by write_png)")
    return rows[:, 1:].reshape(h, w, 3).copy()


def write_apng(path: str, frames, fps=10) -> None:
    """frames (N, H, W, 3) uint8 (numpy, tensor or a list of images) -> an animated PNG (APNG 1.0) that loops for ever at `fps` frames a
    second, written with zlib and struct only: IHDR, acTL, then per frame an fcTL (full size, delay 1 / fps as delay_num / delay_den)
    and the image - frame 0 as IDAT, so a reader that knows nothing of APNG (read_png included) shows the first frame, the others as
    fdAT.  The fcTL and fdAT chunks share one sequence that counts from 0."""
    from fractions import Fraction

    a = frames.detach().cpu().numpy() if hasattr(frames, "detach") else np.asarray(frames)
    if a.ndim != 4 or a.shape[3] != 3 or a.dtype != np.uint8 or min(a.shape[:3]) < 1:
        raise ValueError(f"write_apng: expected (N >= 1, H, W, 3) uint8, got {a.shape} {a.dtype}")
    if not float(fps) > 0.0:
        raise ValueError(f"write_apng: fps must be positive, got {fps}")
    delay = 1 / Fraction(fps).limit_denominator(1000)
    if not (1 <= delay.numerator <= 65535 and 1 <= delay.denominator <= 65535):
        raise ValueError(f"write_apng: a delay of 1 / {fps} s does not fit delay_num / delay_den")
    n, h, w = a.shape[:3]
    out = [b"\x89PNG\r\n\x1a\n", _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)), _png_chunk(b"acTL", struct.pack(">II", n, 0))]
    seq = 0
    for k in range(n):
        out.append(_png_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, delay.numerator, delay.denominator, 0, 0)))
        seq += 1
        if k == 0:
            out.append(_png_chunk(b"IDAT", _png_rows(a[k])))
        else:
            out.append(_png_chunk(b"fdAT", struct.pack(">I", seq) + _png_rows(a[k])))
            seq += 1
    out.append(_png_chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(b"".join(out))


def read_apng(path: str):
    """what write_apng wrote -> (frames (N, H, W, 3) uint8, fps as a float); every CRC, the sequence numbers and the frame count of acTL
    are checked (full-size 8-bit RGB frames, filter 0 only: not a general decoder)"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG")
    pos, size, count, seq, images, delays = 8, None, None, 0, [], []
    while pos < len(data):
        (n,), tag = struct.unpack(">I", data[pos: pos + 4]), data[pos + 4: pos + 8]
        body = data[pos + 8: pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n: pos + 12 + n])[0] != (zlib.crc32(tag + body) & 0xFFFFFFFF):
            raise ValueError(f"{path}: bad CRC in chunk {tag!r}")
        if tag == b"IHDR":
            w, h, bits, kind, _, _, interlace = struct.unpack(">IIBBBBB", body)
            if (bits, kind, interlace) != (8, 2, 0):
                raise ValueError(f"{path}: not an 8-bit RGB non-interlaced PNG")
            size = (h, w)
        elif tag == b"acTL":
            count = struct.unpack(">II", body)[0]
        elif tag in (b"fcTL", b"fdAT"):
            if struct.unpack(">I", body[:4])[0] != seq:
                raise ValueError(f"{path}: chunk {tag!r} carries sequence number {struct.unpack('>I', body[:4])[0]}, expected {seq}")
            seq += 1
            if tag == b"fcTL":
                fw, fh, x, y, num, den = struct.unpack(">IIIIHH", body[4:24])
                if (fh, fw, x, y) != size + (0, 0):
                    raise ValueError(f"{path}: a frame that is not the full image")
                delays.append(num / (den or 100))
            else:
                images.append(body[4:])
        elif tag == b"IDAT":
            if images and len(delays) == 1:
                images[0] += body
            else:
                images.append(body)
        pos += 12 + n
    if count is None or count != len(images) or len(delays) != len(images):
        raise ValueError(f"{path}: acTL announces {count} frames, found {len(images)} images and {len(delays)} fcTL chunks")
    h, w = size
    frames = np.empty((count, h, w, 3), np.uint8)
    for k, z in enumerate(images):
        rows = np.frombuffer(zlib.decompress(z), np.uint8).reshape(h, 1 + 3 * w)
        if rows[:, 0].any():
            raise ValueError(f"{path}: filtered rows (not written by write_apng)")
        frames[k] = rows[:, 1:].reshape(h, w, 3)
    return frames, 1.0 / delays[0]


def contact_sheet(frames, cols: int, background=0) -> np.ndarray:
    """frames (N, H, W, 3) uint8 (numpy or tensor), or a list of (H, W, 3) -> (rows * H, cols' * W, 3) with cols' = min(cols, N), row-major,
    the cells past the last frame filled with `background`"""
    a = frames.detach().cpu().numpy() if hasattr(frames, "detach") else np.asarray(frames)
    if a.ndim != 4 or a.shape[3] != 3 or a.shape[0] < 1 or cols < 1:
        raise ValueError(f"contact_sheet: expected (N >= 1, H, W, 3) and cols >= 1, got {a.shape}, cols = {cols}")
    n, h, w = a.shape[:3]
    cols = min(int(cols), n)
    rows = (n + cols - 1) // cols
    sheet = np.full((rows * h, cols * w, 3), background, np.uint8)
    for k in range(n):
        r, c = divmod(k, cols)
        sheet[r * h: (r + 1) * h, c * w: (c + 1) * w] = a[k]
    return sheet


__all__ = ["Camera", "HipRenderer", "look_at_camera", "default_lights", "write_png", "read_png", "write_apng", "read_apng", "contact_colors", "penetration_colors",
           "contact_sheet", "tslrot6d_to_matrix", "AMBIENT"]
