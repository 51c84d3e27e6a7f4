#!/usr/bin/env python
"""Times the two hot paths of the SIV score against the ways the same results were obtained before libtamf_eval.so.  Needs the GPU.

    python tools/siv_bench.py [--reps 5] [--out siv_bench.json]

  voxelising   the 100^3 lattice of a closed mesh: geometry.voxelize_lattice against geometry.mesh_contains on the 10^6 points
               (brute force, every point against every triangle), at F = 1 554 (a subsampled torus), ~20 000 and ~100 000 faces
  scoring      one clip - 8 sampled frames, 2 hands, 2 objects of ~2 * 10^5 interior points - through metrics.siv.clip_siv against the
               per-frame loop over geometry.solid_intersection_volume, timed twice: as a caller of the parent had to write it (rigid
               transform in numpy on the host and an upload of the query points per object, frame and hand, inside the window), and
               with the 32 sets of query points already on the device (the loop's launches and .item() calls alone)
Every figure: device events around a window of back-to-back calls, sized from a first call to last about 50 ms, after one warm-up call
of the same shape; `reps` windows per path, the paths alternating; the per-call median of the windows is reported with min and max.
Results are compared before they are timed: masks and volumes must be identical."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd")):
    sys.path.insert(0, p)


WINDOW_MS = 50.0


def window(fn, calls):
    """per-call milliseconds of `calls` back-to-back calls between two device events"""
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def alternate(fns, reps):
    """-> (per-call times of each fn over `reps` windows, calls per window of each fn); one warm-up call, windows alternating"""
    import torch

    calls = []
    for fn in fns:
        fn()
        torch.cuda.synchronize()
        calls.append(max(1, int(round(WINDOW_MS / max(window(fn, 1), 1e-3)))))
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            out[k].append(window(fn, calls[k]))
    return out, calls


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def torus_mesh(nu, nv):
    from oracle.fixtures import torus

    v, f = torus(nu, nv)
    c, s = np.cos(0.6), np.sin(0.6)
    return (v @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]]).T) * 0.05 + np.array([0.0013, -0.0007, 0.0021]), f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from oakink2_tamf_amd import geometry
    from oakink2_tamf_amd.metrics import siv

    res = {"voxelise": [], "score": None, "device": torch.cuda.get_device_name(0)}
    for nu, nv in ((37, 21), (100, 100), (224, 224)):  # 2 nu nv faces: 1 554, 20 000, 100 352
        v, f = torus_mesh(nu, nv)
        ax = siv.lattice_axes(v, 1.2, 100)
        tk = torch.from_numpy(ax["ticks"]).cuda()
        x, y, z = np.meshgrid(ax["ticks"][:, 0], ax["ticks"][:, 1], ax["ticks"][:, 2], indexing="ij")
        q = torch.from_numpy(np.vstack((x.flatten(), y.flatten(), z.flatten())).T).cuda()
        new = lambda: geometry.voxelize_lattice(ax["verts_centred"], f, tk)  # noqa: E731
        old = lambda: geometry.mesh_contains(ax["verts_centred"], f, q)  # noqa: E731
        assert torch.equal(new().reshape(-1), old()), "masks differ"
        (t_new, t_old), calls = alternate((new, old), a.reps)
        row = {"faces": int(len(f)), "R": 100, "calls_per_window": calls, "voxelize_lattice": stats(t_new), "mesh_contains_1e6_points": stats(t_old)}
        row["speedup"] = row["mesh_contains_1e6_points"]["median_ms"] / row["voxelize_lattice"]["median_ms"]
        print(json.dumps(row), flush=True)
        res["voxelise"].append(row)

    # one clip: 8 sampled frames (len 160 -> frames 0, 20, ..., 140), 2 objects, MANO-sized closed hand (1 554 faces)
    rng = np.random.default_rng(7)
    hv, hf = torus_mesh(37, 21)
    hv = hv * np.array([1.0, 1.3, 0.8])
    T = 160
    gt = np.stack([hv + 0.002 * np.sin(0.05 * t) for t in range(T)]).astype(np.float32)
    rf = (gt * np.float32(1.03)).astype(np.float32)
    lattices = []
    for k in range(2):
        from oracle.fixtures import torus

        ov, of = torus(60 + 10 * k, 40, 1.0, 0.22)  # axis-aligned ring: ~0.21 of its expanded box, ~2e5 of the 1e6 lattice points
        ov = ov * np.array([0.045, 0.04, 0.1 + 0.01 * k]) + np.array([0.0011, -0.0006, 0.0017])
        lattices.append(siv.object_lattice(ov, of))
    traj = np.zeros((2, T, 9), np.float32)
    traj[:, :, 0:3] = rng.normal(scale=0.01, size=(2, T, 3))
    traj[:, :, 3:9] = rng.normal(size=(2, T, 6))
    new = lambda: siv.clip_siv(gt, rf, hf, traj, lattices, T)  # noqa: E731
    tf = siv.tslrot6d_to_transf(traj)

    def query_points(fr):
        out = []
        for k, l in enumerate(lattices):
            M = tf[k, fr, :3, :].astype(np.float64)
            p = l.points_in
            out.append(torch.from_numpy(np.stack([((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + M[r, 3] for r in range(3)],
                                                 axis=1)).cuda())
        return out

    resident = {fr: query_points(fr) for fr in range(0, T, 20)}  # (both hands of a frame share the query points)

    def loop(points_of):
        out = ([], [])
        for fr in range(0, T, 20):
            for h, hand in enumerate((gt, rf)):
                out[h].append(geometry.solid_intersection_volume(hand[fr], hf, points_of(fr), [l.el_vol for l in lattices]))
        return out

    old = lambda: loop(query_points)  # noqa: E731
    old_resident = lambda: loop(resident.__getitem__)  # noqa: E731
    g_new, g_old, g_res = new(), old(), old_resident()
    assert [float(x) for x in g_new[0]] == g_old[0] == g_res[0] and [float(x) for x in g_new[1]] == g_old[1] == g_res[1], "volumes differ"
    (t_new, t_old, t_res), calls = alternate((new, old, old_resident), a.reps)
    row = {"frames": 8, "hands": 2, "objects": 2, "interior_points": [int(len(l.points_in)) for l in lattices], "hand_faces": int(len(hf)),
           "mean_gt_siv_cm3": float(np.mean(g_new[0])), "calls_per_window": calls, "clip_siv": stats(t_new), "per_frame_loop": stats(t_old),
           "per_frame_loop_points_resident": stats(t_res)}
    row["speedup"] = row["per_frame_loop"]["median_ms"] / row["clip_siv"]["median_ms"]
    row["speedup_vs_points_resident"] = row["per_frame_loop_points_resident"]["median_ms"] / row["clip_siv"]["median_ms"]
    print(json.dumps(row), flush=True)
    res["score"] = row
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
