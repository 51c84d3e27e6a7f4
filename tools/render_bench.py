"""How long rendering a clip takes on the device (libtamf_render.so through render.HipRenderer): ms per 160-frame clip at 512 x 512 of a
hand (1 554 faces, per-frame vertices, smooth shading) and two objects with per-frame poses - as meshes of 20 000 and 100 352 faces, and
again as point clouds of 8 192 points each - plus the time of the rasteriser's launches alone.  The mesh clip is measured three ways in
the same process: as it always was (one opaque layer), with the objects see-through and `--layers` (4) peeled layers, and with that and
`--ssaa` (2) x (2) sub-samples a pixel; and the hand's peel pass (tamf_render_raster_behind) beside its plain raster pass.

    python tools/render_bench.py [--frames 160] [--width 512] [--height 512] [--warmup 2] [--reps 5] [--layers 4] [--ssaa 2] [--obj_alpha 0.4]
                                 [--out render_bench.json]

Times are device events around the enqueued work, ended by a synchronise, after warm-up passes of the same shapes; the median and the
spread (min, max) over --reps are printed, one JSON line.  Needs a GPU: there is no fall-back, and a CPU run says nothing about speed.
The frames stay on the device: reading them back and writing PNG files (launch/render_samples.py) is host work and is not timed here."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def uv_sphere(rings: int, segs: int, radius: float):
    """closed UV sphere: 2 + rings * segs vertices, 2 * rings * segs faces"""
    th = np.pi * (np.arange(rings) + 1) / (rings + 1)
    ph = 2 * np.pi * np.arange(segs) / segs
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), -np.outer(np.cos(th), np.ones(segs))], axis=-1)
    v = np.concatenate([[[0.0, 0.0, -1.0]], ring.reshape(-1, 3), [[0.0, 0.0, 1.0]]]) * radius
    idx = lambda r, s: 1 + r * segs + s % segs  # noqa: E731
    s = np.arange(segs)
    f = [np.stack([np.zeros(segs, int), idx(0, s + 1), idx(0, s)], axis=1)]
    for r in range(rings - 1):
        a, b, c, d = idx(r, s), idx(r, s + 1), idx(r + 1, s), idx(r + 1, s + 1)
        f += [np.stack([a, b, d], axis=1), np.stack([a, d, c], axis=1)]
    f.append(np.stack([np.full(segs, len(v) - 1), idx(rings - 1, s), idx(rings - 1, s + 1)], axis=1))
    return v.astype(np.float32), np.concatenate(f).astype(np.int32)


def poses(F: int, centre, seed: int):
    """(F, 4, 4): a slow rotation about a fixed axis and a drift around `centre`"""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    out = np.tile(np.eye(4), (F, 1, 1))
    for f in range(F):
        a = 0.02 * f
        out[f, :3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
        out[f, :3, 3] = np.asarray(centre) + 0.02 * np.array([np.sin(0.05 * f), np.cos(0.04 * f), np.sin(0.03 * f)])
    return out


def timed(fn, warmup: int, reps: int):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--ssaa", type=int, default=2)
    ap.add_argument("--obj_alpha", type=float, default=0.4)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("render_bench needs a GPU: nothing is measured without one")
    from oakink2_tamf_amd import render as R

    F, W, H = a.frames, a.width, a.height
    rng = np.random.default_rng(0)
    hand_v, hand_f = uv_sphere(21, 37, 0.05)  # 1 554 faces, as the closed MANO hand
    hand = hand_v[None] * np.array([1.0, 0.6, 0.9], np.float32) + (0.002 * rng.normal(size=(F, 1, 3))).astype(np.float32) + np.array([0.09, 0.0, 0.0], np.float32)
    objects = [uv_sphere(100, 100, 0.06), uv_sphere(224, 224, 0.08)]  # 20 000 and 100 352 faces
    assert hand_f.shape[0] == 1554 and [o[1].shape[0] for o in objects] == [20000, 100352]
    centres = [(-0.05, 0.02, 0.03), (0.2, -0.03, 0.06)]
    obj_pose = [poses(F, c, k) for k, c in enumerate(centres)]
    clouds = [(rng.normal(size=(8192, 3)) * r / 2).astype(np.float32) for r in (0.06, 0.08)]
    world = [hand.reshape(-1, 3)] + [np.asarray(c) + np.array([[-0.1, -0.1, -0.1], [0.1, 0.1, 0.1]]) for c in centres]
    cam = R.look_at_camera(np.concatenate(world), W, H)

    def scene(as_points: bool, alpha: float = 1.0):
        rd = R.HipRenderer(W, H, a.device)
        rd.add_mesh(hand, hand_f, color=(0.91, 0.72, 0.60), smooth=True, name="hand")
        for k in range(2):
            if as_points:
                rd.add_points(clouds[k], color=(0.55, 0.8, 0.45), pose=obj_pose[k], point_size=3, alpha=alpha)
            else:
                rd.add_mesh(objects[k][0], objects[k][1], color=(0.55, 0.8, 0.45), pose=obj_pose[k], alpha=alpha)
        return rd

    res = {"frames": F, "width": W, "height": H, "device": torch.cuda.get_device_name(torch.device(a.device)), "warmup": a.warmup, "reps": a.reps,
           "frames_per_chunk": {}}
    for label, as_points in (("meshes", False), ("points", True)):
        rd = scene(as_points)
        res["frames_per_chunk"][label] = rd.frames_per_chunk()
        res[label + "_clip"] = timed(lambda: rd.render(cam), a.warmup, a.reps)
        rgb, depth, prim = rd.render(cam)
        res[label + "_covered_share"] = float((prim >= 0).float().mean())
    # the layered paths beside today's, same process, same scene with see-through objects
    rd = scene(False, a.obj_alpha)
    for label, kw in (("layers", dict(layers=a.layers)), ("layers_ssaa", dict(layers=a.layers, ssaa=a.ssaa))):
        res["frames_per_chunk"]["meshes_" + label] = rd.frames_per_chunk(kw.get("layers", 1), kw.get("ssaa", 1))
        res["meshes_" + label + "_clip"] = dict(timed(lambda: rd.render(cam, **kw), a.warmup, a.reps), **kw)
    # the rasteriser's launches alone, per mesh: projection kept outside the timed window
    lib = R._bind()
    cs = R.camera_struct(cam)
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    depth = torch.empty((F, H, W), dtype=torch.float32, device=a.device)
    prim = torch.empty((F, H, W), dtype=torch.int32, device=a.device)
    import ctypes

    for label, (v, f), pose in (("hand_1554", (hand, hand_f), None), ("object_20000", objects[0], obj_pose[0]), ("object_100352", objects[1], obj_pose[1])):
        vd = torch.from_numpy(np.ascontiguousarray(v)).to(a.device)
        fd = torch.from_numpy(f).to(a.device)
        md = None if pose is None else torch.from_numpy(np.ascontiguousarray(pose[:, :3, :], np.float32)).to(a.device)
        V = int(vd.shape[-2])
        pos = torch.empty((F, V, 3), dtype=torch.float32, device=a.device)
        xy = torch.empty((F, V, 2), dtype=torch.int32, device=a.device)
        R._check(lib, lib.tamf_render_project(P(vd), P(md), ctypes.addressof(cs), F, V, int(vd.dim() == 3), P(pos), P(xy), None))

        def raster():
            R._check(lib, lib.tamf_render_clear(P(depth), P(prim), F, H, W, None))
            R._check(lib, lib.tamf_render_raster(P(xy), P(pos), P(fd), F, V, int(fd.shape[0]), H, W, 0, P(depth), P(prim), None))

        res["raster_" + label] = timed(raster, a.warmup, a.reps)
        floor_d, floor_i = depth.clone(), prim.clone()  # the pass above left layer 0 in depth / prim

        def behind():
            R._check(lib, lib.tamf_render_clear(P(depth), P(prim), F, H, W, None))
            R._check(lib, lib.tamf_render_raster_behind(P(xy), P(pos), P(fd), F, V, int(fd.shape[0]), H, W, 0, P(floor_d), P(floor_i), P(depth), P(prim), None))

        res["raster_behind_" + label] = timed(behind, a.warmup, a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
