"""ms per call of the point-to-mesh distance (libtamf_meshdist.so), culled beside brute force (flag bit 0: every tile visited), at the
SIV bench's mesh sizes - 1 554, 20 000 and 100 352 faces:
    lattice   MeshSet.lattice on the 100^3 lattice of process_sdf (metrics/siv.lattice_axes, bbox_expand_ratio 1.2)
    pd        MeshSet.distance at a clip's PD shape: 8 frames x 2 hands x 2 objects x 778 vertices = 32 jobs, with the inside test
    heat map  MeshSet.distance at the penetration map's shape: 160 frames x 1 hand x 2 objects x 778 vertices = 320 jobs
Device events around each call (the points calls include the host's job packing and its one copy), medians of `--passes` passes after
one warm-up, all in this one process on one box; the two paths are also compared bit for bit.  The meshes are tools/surface_bench.py's
height fields (2 triangles a cell: 21 x 37, 100 x 100 and 224 x 224 cells, 20 x 14 cm); a "hand" is 778 points in a 10 cm ball that
cuts the surface, moved a little from frame to frame.  Preparing a set (validity, Morton order, packing, upload) is timed on the host
clock beside them.

    python tools/meshdist_bench.py [--passes 5] [--json out.json]"""
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
sys.path[:0] = [os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "tools")]

from surface_bench import GRIDS, device_ms, height_field  # noqa: E402

R = 100
N_VERTS = 778
SHAPES = (("pd", 8, 2), ("heat map", 160, 1))  # name, frames, hands


def hands(frames: int, n_hands: int, seed: int) -> np.ndarray:
    """(frames * n_hands * 778, 3) float32: a ball of radius 5 cm centred 1 cm above the height field's middle, drifting 0.5 mm a frame"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(N_VERTS, 3))
    ball = d / np.linalg.norm(d, axis=1, keepdims=True) * (0.05 * rng.uniform(0, 1, (N_VERTS, 1)) ** (1 / 3))
    out = [ball + np.asarray([0.0005 * f, 0.002 * h, 0.01]) for f in range(frames) for h in range(n_hands)]
    return np.concatenate(out).astype(np.float32)


def points_call(ms, frames: int, n_hands: int, cull: bool):
    pts = hands(frames, n_hands, 7)
    slot = np.arange(frames * n_hands, dtype=np.int64).repeat(2)
    obj = np.tile(np.arange(2, dtype=np.int32), frames * n_hands)
    tr = np.tile(np.eye(3, 4).reshape(1, 12), (len(obj), 1))
    tr[obj == 1, 3] = 0.003  # the second object sits 3 mm aside
    dev_pts = torch.from_numpy(pts).to(ms.device)
    return lambda: ms.distance(dev_pts, obj, tr, slot * N_VERTS, np.full(len(obj), N_VERTS, np.int64), inside=True, cull=cull)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from oakink2_tamf_amd.meshdist import MeshSet
    from oakink2_tamf_amd.metrics.siv import lattice_axes

    dev = torch.device("cuda:0")
    pr = torch.cuda.get_device_properties(dev)
    pci = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id) if hasattr(pr, "pci_bus_id") else None
    out = {"device": torch.cuda.get_device_name(dev), "host": socket.gethostname(), "pci": pci, "passes": a.passes, "R": R, "results": []}
    print(f"box {out['host']}, card {pci} ({out['device']}); medians of {a.passes} passes, culled | brute force | culled / brute")
    for nx, ny in GRIDS:
        v, f = height_field(nx, ny)
        ax = lattice_axes(v, 1.2, R)
        t = time.perf_counter()
        one = MeshSet([(ax["verts_centred"], f)], device=dev)
        torch.cuda.synchronize()
        prep = 1e3 * (time.perf_counter() - t)
        two = MeshSet([(v, f), (v, f)], device=dev)
        ticks = torch.from_numpy(ax["ticks"]).to(dev)
        r = {"faces": int(f.shape[0]), "tiles": int(-(-one.perm_off[1] // 64)), "prepare_host_ms": prep}
        cases = [("lattice", lambda c: (lambda: one.lattice(0, ticks, cull=c)))] + [
            (name, (lambda fr, nh: (lambda c: points_call(two, fr, nh, c)))(fr, nh)) for name, fr, nh in SHAPES]
        line = f"F = {r['faces']:6d} ({r['tiles']} tiles, prepared in {prep:.1f} ms on the host):"
        for name, make in cases:
            res = {}
            for label, cull in (("culled", True), ("brute", False)):
                fn = make(cull)
                got = fn()
                res[label + "_out"] = got if isinstance(got, torch.Tensor) else got
                all_ms = device_ms(fn, a.passes)
                res[label + "_ms"], res[label + "_ms_all"] = float(np.median(all_ms)), all_ms
            x, y = res.pop("culled_out"), res.pop("brute_out")
            same = torch.equal(x, y) if isinstance(x, torch.Tensor) else all(torch.equal(p, q) for p, q in zip(x, y))
            res.update(ratio=res["culled_ms"] / res["brute_ms"], same_bits=bool(same))
            r[name] = res
            line += f"  {name} {res['culled_ms']:.3f} | {res['brute_ms']:.3f} ms | {res['ratio']:.3f}{'' if same else ' (BITS DIFFER)'};"
        print(line)
        out["results"].append(r)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
