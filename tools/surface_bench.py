"""ms per object point cloud of surface.sample_point_cloud (libtamf_surface.so: areas + scan + Philox draw + binary search, then
tamf_pointenc_fps) at the SIV bench's mesh sizes - 1 554, 20 000 and 100 352 faces - with 32 768 candidates thinned to 8 192 points,
beside the numpy restatement of the same definition (tests/surface_restatement.py: float64 areas, np.cumsum, Philox in numpy,
np.searchsorted, and the point-encoder tests' host FPS) on the host CPU.  Device events around each call (the call uploads the mesh
and waits for the total area once; both are inside), host clock around the restatement; medians of `--passes` passes after one
warm-up, all in this one process on one box.  The surface samples alone (sample_surface, 32 768 samples) are timed the same way, so
the FPS share shows.  The meshes are height fields over a grid, 2 triangles a cell: 21 x 37, 100 x 100 and 224 x 224 cells.

    python tools/surface_bench.py [--passes 5] [--no_host] [--json out.json]"""
from __future__ import annotations

import argparse
import json
import os
import socket
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests"), ROOT]

GRIDS = ((21, 37), (100, 100), (224, 224))  # 1 554, 20 000, 100 352 faces
N_POINTS, OVERSAMPLE = 8192, 4


def height_field(nx: int, ny: int):
    x, y = np.meshgrid(np.linspace(-0.1, 0.1, nx + 1), np.linspace(-0.07, 0.07, ny + 1), indexing="ij")
    v = np.stack([x, y, 0.02 * np.sin(40.0 * x) * np.cos(55.0 * y)], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    a = (i * (ny + 1) + j).reshape(-1)
    f = np.concatenate([np.stack([a, a + ny + 1, a + ny + 2], 1), np.stack([a, a + ny + 2, a + 1], 1)]).astype(np.int32)
    return v, f


def device_ms(fn, passes: int):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def host_ms(fn, passes: int):
    ms = []
    for _ in range(passes):
        t = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--no_host", action="store_true", help="skip the numpy restatement")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from oakink2_tamf_amd import surface as S

    dev = torch.device("cuda:0")
    pr = torch.cuda.get_device_properties(dev)
    pci = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id) if hasattr(pr, "pci_bus_id") else None
    out = {"device": torch.cuda.get_device_name(dev), "host": socket.gethostname(), "pci": pci, "passes": a.passes, "n_points": N_POINTS,
           "n_candidates": N_POINTS * OVERSAMPLE, "results": []}
    print(f"box {out['host']}, card {pci} ({out['device']}); {N_POINTS * OVERSAMPLE} candidates -> {N_POINTS} points, medians of {a.passes} passes")
    for nx, ny in GRIDS:
        v, f = height_field(nx, ny)
        key = S.object_key(f"grid{nx}x{ny}")
        cloud = device_ms(lambda: S.sample_point_cloud(v, f, N_POINTS, OVERSAMPLE, seed=1, key=key, device=dev), a.passes)
        draw = device_ms(lambda: S.sample_surface(v, f, N_POINTS * OVERSAMPLE, seed=1, key=key, device=dev), a.passes)
        r = {"faces": int(f.shape[0]), "verts": int(v.shape[0]), "cloud_ms": float(np.median(cloud)), "cloud_ms_all": cloud,
             "samples_ms": float(np.median(draw)), "samples_ms_all": draw}
        line = f"F = {r['faces']:6d}: sample_point_cloud {r['cloud_ms']:.3f} ms, of which the {N_POINTS * OVERSAMPLE} surface samples {r['samples_ms']:.3f} ms"
        if not a.no_host:
            import surface_restatement as SR

            got = S.sample_point_cloud(v, f, N_POINTS, OVERSAMPLE, seed=1, key=key, device=dev, faces_out=True)
            idx, ref = SR.point_cloud(v, f, N_POINTS, OVERSAMPLE, 1, key)
            r["equal_to_restatement"] = bool(np.array_equal(got[1].cpu().numpy(), ref["face"][idx]) and np.array_equal(got[0].cpu().numpy(), ref["point"][idx]))
            host = host_ms(lambda: SR.point_cloud(v, f, N_POINTS, OVERSAMPLE, 1, key), a.passes)
            hdraw = host_ms(lambda: SR.sample(v, f, N_POINTS * OVERSAMPLE, 1, key), a.passes)
            r.update(host_cloud_ms=float(np.median(host)), host_cloud_ms_all=host, host_samples_ms=float(np.median(hdraw)), host_samples_ms_all=hdraw)
            line += f"; numpy restatement {r['host_cloud_ms']:.0f} ms, of which the samples {r['host_samples_ms']:.1f} ms; same cloud: {r['equal_to_restatement']}"
        print(line)
        out["results"].append(r)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
