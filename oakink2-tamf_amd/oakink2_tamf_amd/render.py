"""Offscreen rendering of hand / object clips on the GPU (libtamf_render.so, include/tamf_render.h): stands where the reference's
viewers (script/viz_seg.py, script/debug/debug_*_sample.py) and dev_fn/util/vis_pyrender_util.py:PyMultiObjRenderer need Open3D or
pyrender with OpenGL and a display.

HipRenderer      meshes and point clouds with static or per-frame vertices and an optional per-frame rigid pose -> rgb, depth, prim_id
look_at_camera   one fixed pinhole camera per clip, fitted in float64 to the bounding sphere of everything in it
default_lights   the arrangement of PyMultiObjRenderer._create_raymond_lights in this package's camera frame; ambient 0.2
write_png        zlib + struct only: no imaging package at run time
contact_sheet    frames tiled into one image

The image is this package's own rasterisation and Lambert shading, NOT pyrender's PBR output: no textures, no anti-aliasing, no
clipping (a triangle with a vertex in front of the near plane is dropped).  No CPU or torch fall-back for the kernels."""
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

    def add_mesh(self, verts, faces, color=(0.8, 0.8, 0.8), pose=None, smooth: bool = False, name: str = "mesh") -> int:
        """verts (V, 3) static or (F, V, 3) per frame; faces (Nf, 3); pose None, (F, 4, 4) / (F, 3, 4) or (F, 9) tslrot6d rows, applied
        to the vertices before the camera; smooth: shade with geometry.vertex_normals instead of face normals -> the item's index.
        The face indices are range-checked here, once."""
        import torch

        v, m, frames = self._verts(verts, pose, name)
        f = np.asarray(faces.detach().cpu().numpy() if hasattr(faces, "detach") else faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
            raise ValueError(f"{name}: faces must be (Nf, 3) with Nf >= 1, got {f.shape}")
        V = int(v.shape[-2])
        if int(f.min()) < 0 or int(f.max()) >= V:
            raise ValueError(f"{name}: face indices outside [0, {V}) (min {int(f.min())}, max {int(f.max())})")
        f32 = np.ascontiguousarray(f, np.int32)
        self.items.append(_Item("mesh", v, m, torch.from_numpy(f32).to(v.device), f32, _floats(color, 3), bool(smooth), 0, frames))
        return len(self.items) - 1

    def add_points(self, points, color=(0.8, 0.8, 0.8), pose=None, point_size: int = 3, name: str = "points") -> int:
        """points (P, 3) or (F, P, 3); each is drawn as an unlit square of point_size (odd, 1 .. 15) pixels -> the item's index"""
        if point_size % 2 != 1 or not 1 <= point_size <= MAX_POINT_SIZE:
            raise ValueError(f"{name}: point_size must be odd and lie in [1, {MAX_POINT_SIZE}], got {point_size}")
        v, m, frames = self._verts(points, pose, name)
        self.items.append(_Item("points", v, m, None, None, _floats(color, 3), False, int(point_size), frames))
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

    def frames_per_chunk(self) -> int:
        """frames rendered per pass: xy (8 B) + pos_cam (12 B) per vertex and frame, + 12 B of normals for smooth meshes"""
        per_frame = sum(int(it.verts.shape[-2]) * (32 if it.smooth else 20) for it in self.items)
        return max(1, min(65535, PROJECTION_BYTES // max(1, per_frame), (2 ** 31 - 1) // (self.width * self.height)))

    # -- render --------------------------------------------------------------------------------------------------------------
    def render(self, camera: Camera, frames: Optional[Sequence[int]] = None):
        """-> (rgb (F, H, W, 3) uint8, depth (F, H, W) float32 with +inf where nothing was drawn, prim_id (F, H, W) int32 with -1 there)
        device tensors; `frames`: the frame indices to render (default: all)."""
        import torch

        from .hip_backend import _stream_ptr, require_gpu

        if not self.items:
            raise ValueError("nothing to render: add a mesh or a point cloud first")
        if sum(self.counts) > 2 ** 31 - 1:
            raise ValueError("more than 2^31 - 1 primitives")
        dev = require_gpu(self.device)
        total = self.n_frames()
        sel = list(range(total)) if frames is None else [int(i) for i in frames]
        if any(not 0 <= i < total for i in sel):
            raise ValueError(f"frame index outside [0, {total})")
        H, W = self.height, self.width
        rgb = torch.empty((len(sel), H, W, 3), dtype=torch.uint8, device=dev)
        depth = torch.empty((len(sel), H, W), dtype=torch.float32, device=dev)
        prim = torch.empty((len(sel), H, W), dtype=torch.int32, device=dev)
        step = self.frames_per_chunk()
        for s in range(0, len(sel), step):
            part = sel[s: s + step]
            self._render_chunk(camera, part, rgb[s: s + len(part)], depth[s: s + len(part)], prim[s: s + len(part)], dev, _stream_ptr(dev))
        return rgb, depth, prim

    def _render_chunk(self, camera, part, rgb, depth, prim, dev, stream):
        import torch

        lib = _bind()
        F, H, W = len(part), self.height, self.width
        cam = camera_struct(camera)
        idx = torch.as_tensor(part, dtype=torch.long, device=dev)
        P = lambda t: None if t is None else c_void_p(t.data_ptr())  # noqa: E731
        H_ = lambda a: a.ctypes.data_as(c_void_p)  # noqa: E731
        with torch.cuda.device(dev):
            _check(lib, lib.tamf_render_clear(P(depth), P(prim), F, H, W, stream))
            staged = []
            for it, base in zip(self.items, self.prim_base):
                per_frame = it.verts.dim() == 3
                v = it.verts.index_select(0, idx).contiguous() if per_frame else it.verts
                V = int(v.shape[-2])
                model = None if it.pose is None else torch.from_numpy(np.ascontiguousarray(it.pose[part], np.float32)).to(dev)
                pos = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
                xy = torch.empty((F, V, 2), dtype=torch.int32, device=dev)
                _check(lib, lib.tamf_render_project(P(v), P(model), ctypes.addressof(cam), F, V, int(per_frame), P(pos), P(xy), stream))
                if it.kind == "mesh":
                    _check(lib, lib.tamf_render_raster(P(xy), P(pos), P(it.faces), F, V, int(it.faces.shape[0]), H, W, base, P(depth), P(prim), stream))
                else:
                    _check(lib, lib.tamf_render_points(P(xy), P(pos), F, V, H, W, it.point_size, base, P(depth), P(prim), stream))
                staged.append((it, base, v, model, pos, xy))
            for it, base, v, model, pos, xy in staged:
                if it.kind == "mesh":
                    normals = self._camera_normals(it, v, model, camera, F, dev) if it.smooth else None
                    _check(lib, lib.tamf_render_shade_mesh(P(prim), P(xy), P(pos), P(normals), P(it.faces), F, int(v.shape[-2]), int(it.faces.shape[0]), H, W,
                                                           base, H_(it.color), self.ambient, H_(self.lights), int(self.lights.shape[0]), P(rgb), stream))
                else:
                    _check(lib, lib.tamf_render_shade_points(P(prim), F, H, W, base, int(v.shape[-2]), H_(it.color), P(rgb), stream))
            _check(lib, lib.tamf_render_fill(P(prim), F, H, W, H_(self.background), P(rgb), stream))

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


# ---- images ---------------------------------------------------------------------------------------------------------------------
def write_png(path: str, rgb) -> None:
    """(H, W, 3) uint8 (numpy or tensor) -> an 8-bit RGB PNG, written with zlib and struct only"""
    a = rgb.detach().cpu().numpy() if hasattr(rgb, "detach") else np.asarray(rgb)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: expected (H, W, 3) uint8, got {a.shape} {a.dtype}")
    h, w = a.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), np.ascontiguousarray(a).reshape(h, w * 3)], axis=1).tobytes()  # filter 0 per row

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


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


__all__ = ["Camera", "HipRenderer", "look_at_camera", "default_lights", "write_png", "read_png", "contact_sheet", "tslrot6d_to_matrix", "AMBIENT"]
