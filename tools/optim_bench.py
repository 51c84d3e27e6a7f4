"""ms per optimiser step of HipAdamW (libtamf_optim.so: per-parameter clip + AdamW in two launches) beside the reference's sequence -
one torch.nn.utils.clip_grad_norm_(param, 0.1, 2.0) per parameter, then torch.optim.AdamW.step() on PyTorch-ROCm's default (foreach)
path - on the parameter sets of config/arch_mdm_l.yml (the denoiser G) and config/arch_refine.yml (the refiner R), with random
gradients at a scale where some tensors are clipped and some are not.  Both sides run in this one process on one device, in
alternating windows (hip, torch, hip, torch, ...): device events around each call after `--warmup`, every window at least `--seconds`
long; per side the median and the 10th / 90th percentiles over all of its windows, and each window's median (drift of the box shows
as a trend over the windows).  Also: the bytes the HIP step moves (the norm pass reads g; the update reads p, g, m, v and writes p, m,
v: 8 float32 streams) over its median time, against the measured and the datasheet HBM rate.

The torch side restores its gradients before every call (clip_grad_norm_ scales them in place); that copy is outside its events.

    python tools/optim_bench.py [--rounds 3] [--seconds 1.0] [--warmup 5] [--json out.json]"""
from __future__ import annotations

import argparse
import json
import os
import socket
import sys

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oakink2-tamf_amd")]

HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0  # float4 copy on this chip / the datasheet


def parameter_shapes(name: str):
    with open(os.path.join(ROOT, "config", name)) as f:
        mc = yaml.safe_load(f)["model"]
    if name == "arch_refine.yml":
        from oakink2_tamf_amd.model.segment_refine_model import SegmentRefineModel

        model = SegmentRefineModel(None, **mc, use_pc=True)
    else:
        from oakink2_tamf_amd.model.interaction_segment_mdm import InterationSegmentMDM

        model = InterationSegmentMDM(**mc)
    return [tuple(p.shape) for k, p in model.named_parameters() if not k.startswith("clip_model.")]


def window(fn, before, seconds, warmup):
    """-> [ms per call]: calls of fn between device events until the window has run for `seconds`; before() runs outside the events"""
    for _ in range(warmup):
        before()
        fn()
    torch.cuda.synchronize()
    ms = []
    while sum(ms) < 1e3 * seconds or len(ms) < 10:
        before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def stats(ms):
    return [float(np.median(ms)), float(np.percentile(ms, 10)), float(np.percentile(ms, 90))]


def bench(name: str, rounds: int, seconds: float, warmup: int, dev) -> dict:
    from oakink2_tamf_amd.optim import HipAdamW

    shapes = parameter_shapes(name)
    g = torch.Generator(device="cpu").manual_seed(0)
    init = [0.05 * torch.randn(s, generator=g) for s in shapes]
    grads = [(torch.randn(s, generator=g) * 10.0 ** float(torch.empty(1).uniform_(-3, 0, generator=g)) / np.sqrt(max(1, int(np.prod(s))))).to(dev)
             for s in shapes]
    hip_p = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    tor_p = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    for p, gr in zip(hip_p, grads):
        p.grad = gr.clone()
    for p, gr in zip(tor_p, grads):
        p.grad = gr.clone()
    hip_opt = HipAdamW(hip_p, lr=1e-4, weight_decay=0.0, clip_max_norm=0.1)
    tor_opt = torch.optim.AdamW(tor_p, lr=1e-4, weight_decay=0.0)

    def torch_step():
        for p in tor_p:
            torch.nn.utils.clip_grad_norm_(p, 0.1, 2.0)
        tor_opt.step()

    def restore():
        torch._foreach_copy_([p.grad for p in tor_p], grads)

    sides = {"hip": [], "torch": []}
    for _ in range(rounds):
        sides["hip"].append(window(hip_opt.step, lambda: None, seconds, warmup))
        sides["torch"].append(window(torch_step, restore, seconds, warmup))
    numel = int(sum(np.prod(s) for s in shapes))
    res = {"config": name, "tensors": len(shapes), "parameters": numel, "rounds": rounds, "seconds": seconds}
    for side, wins in sides.items():
        allms = [x for w in wins for x in w]
        res[side + "_ms"], res[side + "_ms_p10"], res[side + "_ms_p90"] = stats(allms)
        res[side + "_calls"] = len(allms)
        res[side + "_window_medians_ms"] = [float(np.median(w)) for w in wins]
    res["torch_over_hip"] = res["torch_ms"] / res["hip_ms"]
    res["intervals_overlap"] = not (res["hip_ms_p90"] < res["torch_ms_p10"] or res["torch_ms_p90"] < res["hip_ms_p10"])
    moved = 8 * 4 * numel
    res["hip_bytes_moved"] = moved
    res["hip_tb_per_s"] = moved / (res["hip_ms"] * 1e-3) / 1e12
    res["hip_fraction_of_measured_hbm"] = res["hip_tb_per_s"] / HBM_MEASURED_TBS
    res["hip_fraction_of_spec_hbm"] = res["hip_tb_per_s"] / HBM_SPEC_TBS
    hip_opt.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)  # (a window of a fraction of a second measures the scheduler)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pr = torch.cuda.get_device_properties(dev)
    pci = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id) if hasattr(pr, "pci_bus_id") else None
    out = {"device": torch.cuda.get_device_name(dev), "host": socket.gethostname(), "pci": pci, "results": [bench(n, a.rounds, a.seconds, a.warmup, dev) for n in ("arch_mdm_l.yml", "arch_refine.yml")]}
    print(f"box {out['host']}, card {out['pci']} ({out['device']})")
    for r in out["results"]:
        print(f"{r['config']}: {r['tensors']} tensors, {r['parameters'] / 1e6:.2f} M parameters")
        for side in ("hip", "torch"):
            print(f"  {side:5s} {r[side + '_ms']:.4f} ms [{r[side + '_ms_p10']:.4f}, {r[side + '_ms_p90']:.4f}] over {r[side + '_calls']} calls; "
                  f"window medians {['%.4f' % m for m in r[side + '_window_medians_ms']]}")
        print(f"  torch / hip = {r['torch_over_hip']:.2f}x; intervals overlap: {r['intervals_overlap']}; hip moves {r['hip_bytes_moved'] / 1e9:.3f} GB "
              f"at {r['hip_tb_per_s']:.2f} TB/s = {100 * r['hip_fraction_of_measured_hbm']:.0f} % of {HBM_MEASURED_TBS} TB/s measured "
              f"({100 * r['hip_fraction_of_spec_hbm']:.0f} % of {HBM_SPEC_TBS} TB/s spec)")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
