#!/usr/bin/env python
"""Times the SDF-lattice sampler (sdfgrid.penetration_depth: forward, and forward + backward) at the training shape - 64 clips, 160
frames, 2 objects, 778 hand vertices, two lattices of R = 100 - beside a torch assembly of the same quantity on the same device: the
float32 Gram-Schmidt and inverse pose in torch ops, then one torch.nn.functional.grid_sample (trilinear, align_corners=True, zero
padding) per lattice over all clips' vertices, relu, and autograd for the backward.  Needs the GPU.

    python tools/sdfgrid_bench.py [--reps 5] [--out sdfgrid_bench.json]

Every figure: device events around a window of back-to-back calls, sized from a first call to last about 50 ms, after one warm-up call
of the same shape; `reps` windows per path, the paths alternating; the per-call median of the windows is reported with min and max.
The two are compared before they are timed (float32 assembly against the float64 kernel: within 1e-5 of the lattice's largest value).

Also printed: the largest |lattice depth - exact depth| over a hand-sized cloud (778 points) pushed into a sphere mesh, the lattice
from meshdist.process_sdf at R = 100, the exact depth from MeshSet.distance with its inside test: what the lattice's resolution costs."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)

from siv_bench import alternate, stats  # noqa: E402

EPS = float(np.finfo(np.float32).eps)


def sphere_mesh(radius=0.05, n=48):
    """a closed UV sphere of 9 024 faces, turned out of the lattice's axes: with its poles on the z axis the vertical rays of the inside
    test run exactly through mesh edges on the columns |x| = |y|, where check_mesh_contains (the sign of process_sdf) then calls
    interior lattice points outside - 1 842 of 294 192 on this mesh"""
    th = np.linspace(0, np.pi, n + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, 2 * n, endpoint=False)
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones_like(ph))], -1).reshape(-1, 3)
    v = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]]) * radius
    m, faces = 2 * n, []
    for j in range(m):
        faces.append([0, 1 + j, 1 + (j + 1) % m])
        faces.append([len(v) - 1, 1 + (n - 2) * m + (j + 1) % m, 1 + (n - 2) * m + j])
    for i in range(n - 2):
        for j in range(m):
            a, b = 1 + i * m + j, 1 + i * m + (j + 1) % m
            faces += [[a, a + m, b + m], [a, b + m, b]]
    (c1, s1), (c2, s2) = (np.cos(0.6), np.sin(0.6)), (np.cos(0.37), np.sin(0.37))
    turn = np.array([[1, 0, 0], [0, c1, -s1], [0, s1, c1]]) @ np.array([[c2, -s2, 0], [s2, c2, 0], [0, 0, 1]])
    return v @ turn.T, np.asarray(faces, np.int32)


def grid_sample_depth(grids, hv, tr):
    """the same depth from torch ops, float32: object o of every clip reads lattice o.  hv (B,T,V,3), tr (B,nobj,T,9) -> (B,nobj,T,V)"""
    import torch
    import torch.nn.functional as F

    values, grid_off, res, origin, step = grids.tensors()
    a1, a2 = tr[..., 3:6], tr[..., 6:9]
    b1 = a1 / a1.norm(dim=-1, keepdim=True).clamp_min(EPS)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = b2 / b2.norm(dim=-1, keepdim=True).clamp_min(EPS)
    R = torch.stack([b1, b2, torch.linalg.cross(b1, b2)], dim=-2)  # (B, nobj, T, 3, 3) rows
    d = hv[:, None] - tr[:, :, :, None, 0:3]  # (B, nobj, T, V, 3)
    p = torch.einsum("botrk,botvr->botvk", R, d)
    out = []
    for o in range(tr.shape[1]):
        r = int(res[o])
        vol = values[int(grid_off[o]):int(grid_off[o]) + r ** 3].reshape(1, 1, r, r, r)
        u = (p[:, o] - origin[o].float()) / (step[o].float() * (r - 1)) * 2.0 - 1.0  # in [-1, 1] over the lattice
        g = u.flip(-1).reshape(1, -1, 1, 1, 3)  # grid_sample's x is the last lattice axis
        s = F.grid_sample(vol, g, mode="bilinear", padding_mode="zeros", align_corners=True).reshape(p[:, o].shape[:-1])
        inside = ((u >= -1) & (u <= 1)).all(-1)
        out.append(torch.relu(s) * inside)
    return torch.stack(out, dim=1)


def timings(reps):
    import torch

    import sdfgrid_cases as C
    from oakink2_tamf_amd import sdfgrid

    B, T, nobj, V, R = 64, 160, 2, 778, 100
    fields = [C.fields_from(C.sphere_fn(0.05), [0, 0, 0], [0.15, 0.14, 0.16], R), C.fields_from(C.sphere_fn(0.04, (0.01, 0, 0)), [0.01, 0, 0], [0.12, 0.13, 0.11], R)]
    grids = sdfgrid.SdfGridSet(fields, device="cuda:0")
    g = torch.Generator().manual_seed(0)
    hv = (0.04 * torch.randn(B, T, V, 3, generator=g)).cuda()  # a hand-sized cloud around the objects: about half the vertices inside a lattice
    tr = torch.cat([0.01 * torch.randn(B, nobj, T, 3, generator=g), torch.randn(B, nobj, T, 6, generator=g)], dim=-1).cuda()
    up = torch.randn(B, nobj, T, V, generator=g).cuda()
    gid = torch.arange(nobj, dtype=torch.int32).expand(B, nobj).contiguous().cuda()
    with torch.no_grad():
        got, want = grids.penetration_depth(hv, tr, gid), grid_sample_depth(grids, hv, tr)
    top = float(np.abs(grids.values).max())
    err = float((got - want).abs().max())
    assert err <= 1e-5 * max(top, 1.0) + 1e-6, f"the two paths differ by {err}"

    def fwd_k():
        with torch.no_grad():
            grids.penetration_depth(hv, tr, gid)

    def fwd_t():
        with torch.no_grad():
            grid_sample_depth(grids, hv, tr)

    def fb_k():
        x = hv.detach().clone().requires_grad_(True)
        (grids.penetration_depth(x, tr, gid) * up).sum().backward()

    def fb_t():
        x = hv.detach().clone().requires_grad_(True)
        (grid_sample_depth(grids, x, tr) * up).sum().backward()

    (t_fk, t_ft, t_bk, t_bt), calls = alternate((fwd_k, fwd_t, fb_k, fb_t), reps)
    row = {"shape": "training", "B": B, "T": T, "nobj": nobj, "V": V, "R": R, "samples": B * T * nobj * V, "fraction_positive": float((got > 0).float().mean()),
           "max_abs_difference_of_the_paths": err, "calls_per_window": calls, "kernels_forward": stats(t_fk), "kernels_forward_backward": stats(t_bk),
           "grid_sample_forward": stats(t_ft), "grid_sample_forward_backward": stats(t_bt)}
    row["speedup_forward"] = row["grid_sample_forward"]["median_ms"] / row["kernels_forward"]["median_ms"]
    row["speedup_forward_backward"] = row["grid_sample_forward_backward"]["median_ms"] / row["kernels_forward_backward"]["median_ms"]
    print(json.dumps(row), flush=True)
    return row


def accuracy():
    """lattice depth against exact depth for a hand-sized cloud pushed into a sphere mesh"""
    import torch

    from oakink2_tamf_amd import meshdist, sdfgrid

    v, f = sphere_mesh()
    fields = meshdist.process_sdf(v, f, resolution=100, device="cuda:0")
    grids = sdfgrid.SdfGridSet([fields], device="cuda:0")
    rng = np.random.default_rng(1)
    pts = (rng.normal(size=(778, 3)) * 0.03 + np.array([0.03, 0.0, 0.0])).astype(np.float32)  # a cloud 6 cm wide, its centre 3 cm off the sphere's
    identity = torch.tensor([0, 0, 0, 1, 0, 0, 0, 1, 0], dtype=torch.float32).reshape(1, 1, 1, 9).cuda()
    lattice = grids.penetration_depth(torch.from_numpy(pts).reshape(1, 1, -1, 3).cuda(), identity, torch.zeros(1, 1, dtype=torch.int32)).reshape(-1).double()
    dist, _, inside = meshdist.MeshSet([(v, f)], device="cuda:0").distance(torch.from_numpy(pts).cuda(), [0], inside=True)
    exact = torch.where(inside, dist, torch.zeros_like(dist))
    diff = (lattice - exact).abs()
    # who is right where the two differ: the sphere's own depth r - |p| (the mesh is inscribed: its surface lies up to 0.03 mm inside)
    analytic = torch.from_numpy(np.maximum(0.05 - np.linalg.norm(pts.astype(np.float64), axis=1), 0.0)).to(diff.device)
    agree = (lattice > 0) == inside
    row = {"mesh_faces": int(len(f)), "radius_m": 0.05, "R": 100, "step_m": [float(s) for s in grids.step[0]], "points": 778, "points_inside": int(inside.sum()),
           "max_abs_lattice_minus_exact_m": float(diff.max()), "mean_abs_lattice_minus_exact_m": float(diff.mean()),
           "max_exact_depth_m": float(exact.max()), "points_where_inside_disagrees": int((~agree).sum()),
           "max_abs_lattice_minus_exact_where_inside_agrees_m": float(diff[agree].max()),
           "max_abs_lattice_minus_analytic_m": float((lattice - analytic).abs().max()), "max_abs_exact_minus_analytic_m": float((exact - analytic).abs().max()),
           "lattice_nodes_positive": int((grids.values > 0).sum()), "lattice_nodes_inside_the_sphere": int((np.linalg.norm(np.asarray(fields["point"]), axis=1) < 0.05).sum())}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    res = {"device": torch.cuda.get_device_name(0), "accuracy": accuracy(), "rows": [timings(a.reps)]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
