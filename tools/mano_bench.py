#!/usr/bin/env python3
"""Time the native MANO layer (HipManoLayer) against the float32 torch restatement of the same definition (tests/mano_restatement.py,
its tensors on the device), same box, same process, alternating, HIP events after a warm-up.

    python tools/mano_bench.py [--reps 30] [--rounds 5] [--out mano_bench.json]

Shapes: N = 196 (one clip), 64 x 196 (the refine benchmark's batch) and 2 x 64 x 196 hands per call, on synthetic MANO-shaped arrays
(tests/mano_fixture.py).  Per shape and per frame-tile choice (16-frame tiles a workgroup keeps per basis fragment: 1, 2, 4): the
median over rounds of the mean ms per call, and the achieved bytes/s against what the kernel must write (N x (778 + 21) x 12 B).
The torch restatement is NOT manotorch (which is not available to this project); its time is the time of a chain of torch ops that
compute the same definition, nothing more.

    python tools/mano_bench.py --backward [--reps 30] [--rounds 5] [--out mano_bench_backward.json]

times the gradient instead, at N = 160 (one clip) and 64 x 160 frames, upstream on vertices and joints: tamf_mano_backward alone, the
HIP forward + backward through autograd (HipManoLayer(differentiable=True): loss, .backward()), and torch autograd through the float32
restatement on the same device (forward + backward, the same loss), alternating in the same run."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def timed(fn, reps):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_backward(a, arrays, hip, ref, dev):
    """the gradient at N = 160 and 64 x 160 frames -> rows"""
    import numpy as np
    import torch

    import mano_fixture as F
    from oakink2_tamf_amd.mano import HipManoLayer

    rows = []
    diff = HipManoLayer(arrays, 0, dev, differentiable=True)
    for N in (160, 64 * 160):
        q, b = F.random_inputs(N)
        q, b = torch.from_numpy(q).float().to(dev).requires_grad_(True), torch.from_numpy(b).float().to(dev).requires_grad_(True)
        g = torch.Generator().manual_seed(0)
        gv, gj = torch.randn(N, 778, 3, generator=g).to(dev), torch.randn(N, 21, 3, generator=g).to(dev)
        qd, bd = q.detach(), b.detach()

        def through(layer):
            def run():
                q.grad = b.grad = None
                out = layer(pose_coeffs=q, betas=b)
                ((out.verts * gv).sum() + (out.joints * gj).sum()).backward()
            return run

        variants = [("hip_backward_only", lambda: hip.backward_raw(qd, bd, gv, gj)), ("hip_forward_only", lambda: hip(pose_coeffs=qd, betas=bd)),
                    ("hip_forward_backward_autograd", through(diff)), ("torch_f32_restatement_forward_backward_autograd", through(ref))]
        ms = {name: [] for name, _ in variants}
        for _, fn in variants:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):  # alternating
            for name, fn in variants:
                ms[name].append(timed(fn, a.reps))
        for name, _ in variants:
            row = {"N": N, "variant": name, "ms_median": float(np.median(ms[name])), "ms_min": float(min(ms[name])), "ms_max": float(max(ms[name]))}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def bench_forward(a, arrays, hip, ref, dev):
    """the forward at 196, 64 x 196 and 2 x 64 x 196 hands per call, per frame-tile choice -> rows"""
    import numpy as np
    import torch

    import mano_fixture as F

    rows = []
    for N in (196, 64 * 196, 2 * 64 * 196):
        q, b = F.random_inputs(N)
        q, b = torch.from_numpy(q).float().to(dev), torch.from_numpy(b).float().to(dev)
        variants = [("torch_f32_restatement", lambda: ref(pose_coeffs=q, betas=b), None)]
        for tiles in (1, 2, 4, 0):
            variants.append((f"hip_tiles{tiles}" if tiles else "hip_default", lambda: hip(pose_coeffs=q, betas=b), tiles))
        ms = {name: [] for name, _, _ in variants}
        for name, fn, tiles in variants:  # warm-up of every variant at this shape
            if tiles is not None:
                hip.set_tiles(tiles)
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):  # alternating
            for name, fn, tiles in variants:
                if tiles is not None:
                    hip.set_tiles(tiles)
                ms[name].append(timed(fn, a.reps))
        hip.set_tiles(0)
        out_bytes = N * (778 + 21) * 12
        for name, _, _ in variants:
            med = float(np.median(ms[name]))
            row = {"N": N, "variant": name, "ms_median": med, "ms_min": float(min(ms[name])), "ms_max": float(max(ms[name])),
                   "out_GBps": out_bytes / med / 1e6}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--backward", action="store_true", help="time the gradient (tamf_mano_backward) instead of the forward")
    a = ap.parse_args(argv)
    import torch

    import mano_fixture as F
    import mano_restatement as R
    from oakink2_tamf_amd.mano import HipManoLayer, ManoArrays

    if not torch.cuda.is_available():
        raise SystemExit("mano_bench: no GPU visible; there is nothing to measure on a CPU")
    dev = "cuda:0"
    arrays = ManoArrays(**F.synthetic_arrays(778))
    hip, ref = HipManoLayer(arrays, 0, dev), R.TorchManoLayer(arrays, 0, dev)
    rows = (bench_backward if a.backward else bench_forward)(a, arrays, hip, ref, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
