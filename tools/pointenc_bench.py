"""ms per 8192-point cloud of the native point encoder's three stages (fps, group, encode) beside the same stages restated in
PyTorch-ROCm on the same device (tests/pointenc_fixture.restatement for the encoder; misc.fps / knn_point restated with torch ops),
on seeded weights and clouds.  HIP events around `--iters` calls after `--warmup`; the median is reported.

    python tools/pointenc_bench.py [--clouds 2] [--iters 10] [--warmup 2] [--json out.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")]
import pointenc_fixture as F  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def torch_fps(xyz, G, start):
    B, N, _ = xyz.shape
    idx = torch.zeros(B, G, dtype=torch.long, device=xyz.device)
    dist = torch.full((B, N), 1e10, device=xyz.device)
    far, bi = start.clone(), torch.arange(B, device=xyz.device)
    for i in range(G):
        idx[:, i] = far
        dist = torch.minimum(dist, ((xyz - xyz[bi, far][:, None]) ** 2).sum(-1))
        far = dist.argmax(-1)
    return idx


def torch_group(xyz, centre_idx, M):
    c = torch.gather(xyz, 1, centre_idx[..., None].expand(-1, -1, 3))
    d = -2 * c @ xyz.transpose(1, 2) + (c ** 2).sum(-1)[..., None] + (xyz ** 2).sum(-1)[:, None]
    return d.topk(M, dim=-1, largest=False, sorted=False)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from oakink2_tamf_amd.model.point_encoder import HipPointEncoder

    dev = torch.device("cuda:0")
    cfg, N, _ = F.CASES["full"]
    sd = F.seeded_state_dict(cfg, F.WEIGHT_SEED["full"])
    enc = HipPointEncoder(cfg, device=dev)
    enc.load_state_dict(sd)
    pts = torch.from_numpy(F.seeded_clouds(a.clouds, N, cfg["point_dims"], 5)).to(dev)
    xyz = pts[..., :3].contiguous()
    start = torch.zeros(a.clouds, dtype=torch.long, device=dev)
    centre = enc.fps(pts)
    nbr = enc.group(pts, centre)
    sd_dev = {k: torch.from_numpy(v).to(dev) for k, v in sd.items()}
    res = {"clouds": a.clouds, "points": N, "iters": a.iters}
    with torch.no_grad():
        for name, hip, ref in (
            ("fps", lambda: enc.fps(pts), lambda: torch_fps(xyz, cfg["num_group"], start)),
            ("group", lambda: enc.group(pts, centre), lambda: torch_group(xyz, centre, cfg["group_size"])),
            ("encode", lambda: enc.encode_groups(pts, centre, nbr), lambda: F.restatement(sd_dev, cfg, pts, centre, nbr, torch.float32, dev)),
        ):
            res[name + "_hip_ms_per_cloud"] = timed(hip, a.iters, a.warmup) / a.clouds
            res[name + "_torch_ms_per_cloud"] = timed(ref, a.iters, a.warmup) / a.clouds
        out = enc.encode_groups(pts, centre, nbr)
        ref = F.restatement(sd_dev, cfg, pts, centre, nbr, torch.float32, dev)
        res["max_abs_diff_hip_vs_torch_f32"] = float((out - ref).abs().max())
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
