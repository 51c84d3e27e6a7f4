"""ms per call of the generalized winding number (libtamf_winding.so) at the SIV bench's mesh sizes - 1 554, 20 000 and 100 352 faces:
    lattice   WindingSet.lattice on the 100^3 lattice of process_sdf (metrics/siv.lattice_axes, bbox_expand_ratio 1.2)
    pd        WindingSet.points at a clip's PD shape: 8 frames x 2 hands x 2 objects x 778 vertices = 32 jobs, with the chunks spread over
              work groups (route "spread"), looped over in every thread (route "loop"), and as the library decides (route None)
Device events around each call (the points calls include the host's job packing and its one copy), medians of `--passes` passes after
one warm-up, all in this one process on one box; the routes are also compared bit for bit.  Meshes and hands are tools/meshdist_bench.py's.
Beside them, for scale, the figures committed in DESIGN.md section 4 for the same lattice: the ray-parity voxeliser and meshdist's
brute-force lattice.  The work here is (points x faces) evaluations of a float64 atan2: expect the order of the latter.

    python tools/winding_bench.py [--passes 5] [--json out.json]"""
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

from meshdist_bench import N_VERTS, R, hands  # noqa: E402
from surface_bench import GRIDS, device_ms, height_field  # noqa: E402

VOXELISER_MS = {1554: 0.30, 20000: 2.77, 100352: 13.0}  # geometry.voxelize_lattice, the committed figures
MESHDIST_BRUTE_MS = {1554: 8.70, 20000: 110.0, 100352: 546.0}  # MeshSet.lattice(cull=False), the committed figures
FRAMES, N_HANDS = 8, 2


def points_call(ws, route):
    pts = hands(FRAMES, N_HANDS, 7)
    slot = np.arange(FRAMES * N_HANDS, dtype=np.int64).repeat(2)
    obj = np.tile(np.arange(2, dtype=np.int32), FRAMES * N_HANDS)
    tr = np.tile(np.eye(3, 4).reshape(1, 12), (len(obj), 1))
    tr[obj == 1, 3] = 0.003  # the second object sits 3 mm aside
    dev_pts = torch.from_numpy(pts).to(ws.device)
    return lambda: ws.points(dev_pts, obj, tr, slot * N_VERTS, np.full(len(obj), N_VERTS, np.int64), inside=True, route=route)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from oakink2_tamf_amd.metrics.siv import lattice_axes
    from oakink2_tamf_amd.winding import CHUNK, WindingSet

    dev = torch.device("cuda:0")
    pr = torch.cuda.get_device_properties(dev)
    pci = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id) if hasattr(pr, "pci_bus_id") else None
    out = {"device": torch.cuda.get_device_name(dev), "host": socket.gethostname(), "pci": pci, "passes": a.passes, "R": R, "results": []}
    print(f"box {out['host']}, card {pci} ({out['device']}); medians of {a.passes} passes")
    for nx, ny in GRIDS:
        v, f = height_field(nx, ny)
        F = int(f.shape[0])
        ax = lattice_axes(v, 1.2, R)
        t = time.perf_counter()
        one = WindingSet([(ax["verts_centred"], f)], device=dev)
        torch.cuda.synchronize()
        prep = 1e3 * (time.perf_counter() - t)
        two = WindingSet([(v, f), (v, f)], device=dev)
        ticks = torch.from_numpy(ax["ticks"]).to(dev)
        r = {"faces": F, "chunks": -(-int(one.valid_off[1]) // CHUNK), "prepare_host_ms": prep}
        fn = lambda: one.lattice(0, ticks)  # noqa: E731
        fn()
        all_ms = device_ms(fn, a.passes)
        r["lattice"] = {"ms": float(np.median(all_ms)), "ms_all": all_ms, "voxeliser_ms": VOXELISER_MS.get(F), "meshdist_brute_ms": MESHDIST_BRUTE_MS.get(F),
                        "ns_per_pair": 1e6 * float(np.median(all_ms)) / (R ** 3 * F)}
        line = (f"F = {F:6d} ({r['chunks']} chunks, prepared in {prep:.1f} ms on the host):  lattice {r['lattice']['ms']:.3f} ms "
                f"(ray-parity voxeliser {VOXELISER_MS.get(F)} ms, meshdist brute force {MESHDIST_BRUTE_MS.get(F)} ms);  pd")
        ref = None
        r["pd"] = {}
        for route in ("spread", "loop", None):
            fn = points_call(two, route)
            got = fn()
            all_ms = device_ms(fn, a.passes)
            ref = got if ref is None else ref
            same = torch.equal(got[0].view(torch.int64), ref[0].view(torch.int64)) and torch.equal(got[1], ref[1])
            r["pd"][str(route)] = {"ms": float(np.median(all_ms)), "ms_all": all_ms, "same_bits": bool(same)}
            line += f" {route}: {float(np.median(all_ms)):.3f} ms{'' if same else ' (BITS DIFFER)'}"
        print(line)
        out["results"].append(r)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
