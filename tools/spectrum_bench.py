#!/usr/bin/env python
"""Time tamf_power_spectrum_sum against torch.fft.fft (float64, same device) on the PSKL-J data-path shape.

    python tools/spectrum_bench.py [--n 2048] [--t 160] [--f 63] [--reps 20]

HIP events around one call each, warm (3 untimed calls first), median / min / max of --reps; one JSON line.  The torch yardstick does
what the restatement does on the device: float32 second difference, cast to float64, fft along time, |.|^2, sum over clips."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oakink2-tamf_amd")]


def timed(fn, reps, torch):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def main():
    import torch

    from oakink2_tamf_amd.metrics.psklj import power_spectrum_sum

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--t", type=int, default=160)
    ap.add_argument("--f", type=int, default=63)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(a.n, a.t, a.f, generator=g).cuda()

    def torch_fft():
        acc = torch.diff(x, n=2, dim=1).double()
        s = torch.fft.fft(acc, dim=1)
        return (s.real ** 2 + s.imag ** 2).sum(dim=0)

    def torch_fft_only(acc=torch.diff(x, n=2, dim=1).double()):
        return torch.fft.fft(acc, dim=1)

    res = {"device": torch.cuda.get_device_name(0), "N": a.n, "T": a.t, "F": a.f, "reps": a.reps,
           "tamf_power_spectrum_sum": timed(lambda: power_spectrum_sum(x, chunk=a.n), a.reps, torch),
           "torch_diff_fft64_abs2_sum": timed(torch_fft, a.reps, torch),
           "torch_fft64_alone": timed(torch_fft_only, a.reps, torch)}
    ref = torch_fft()
    got = power_spectrum_sum(x, chunk=a.n)
    res["max_rel_diff_vs_torch"] = float(((got - ref).abs().max(dim=0).values / ref.abs().max(dim=0).values).max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
