"""ms per trunk training step (HIP forward + backward, loss = a fixed cotangent on refine_pose_repr) of the refiner's HIP training step
beside a torch.nn assembly of the same model doing forward + backward through PyTorch-ROCm autograd in fp32 on the same device, in the
same run: config/arch_refine.yml, B = 64 clips of T = 160 frames, 2 objects, dropout 0.1, seeded weights and inputs.  Device events
around each call after `--warmup`; every window runs for at least `--seconds`; the median and the 10th / 90th percentiles are reported,
the HIP side before and after the torch side (drift of the box shows as a difference).  Then, in a window of its own, the per-kernel
breakdown of the HIP step from the library's event profile (tamf_refinetrain_set_profile).  The MANO / nearest-neighbour loss and the
optimiser are left out of both sides (the same code on either).

    python tools/refinetrain_bench.py [--batch 64] [--frames 160] [--nobj 2] [--seconds 1.0] [--warmup 5] [--json out.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")]
import refine_train_restatement as R  # noqa: E402


class TorchRefiner(nn.Module):
    """the refiner trunk's training forward assembled from torch.nn modules"""

    def __init__(self, arch, dropout):
        super().__init__()
        d = arch.latent_dim
        self.shape_embed, self.obj_embed = nn.Linear(arch.hand_shape_dim, d), nn.Linear(arch.obj_embed_dim, d)
        self.pose, self.traj, self.dist = nn.Linear(arch.input_dim, d), nn.Linear(arch.obj_input_dim, d), nn.Linear(arch.h2o_dim, d)
        self.merge = nn.Sequential(nn.Linear(3 * d, d), nn.SiLU(), nn.Linear(d, d))
        layer = nn.TransformerEncoderLayer(d_model=d, nhead=arch.num_heads, dim_feedforward=arch.ff_size, dropout=dropout, activation="gelu")
        self.enc = nn.TransformerEncoder(layer, num_layers=arch.num_layers, enable_nested_tensor=False)
        self.head = nn.Linear(d, arch.input_dim)
        self.drop = nn.Dropout(dropout)

    def forward(self, side, pe, b):
        prefix = torch.nan_to_num(torch.stack([side, self.shape_embed(b["shape"].mean(1)), self.obj_embed(b["obj_embedding"].mean(1))], 0))
        x = self.merge(torch.cat([self.pose(b["sample_pose_repr"]), self.traj(b["obj_traj"]).mean(1), self.dist(b["h2o_dist"])], -1))
        seq = torch.cat([prefix, torch.nan_to_num(x).permute(1, 0, 2)], 0)
        seq = self.drop(seq + pe[: seq.shape[0]])
        return torch.nan_to_num(b["sample_pose_repr"] + self.head(self.enc(seq)[3:]).permute(1, 0, 2))


def timed(fn, seconds, warmup):
    """-> (median, p10, p90 ms, calls): calls of fn between device events until the window has run for `seconds`"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    while sum(ms) < 1e3 * seconds or len(ms) < 10:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.percentile(ms, 10)), float(np.percentile(ms, 90)), len(ms)


def step_flop(arch, B, T, nobj):
    """the multiply-adds of one forward, x 2, from the shapes: (layers' linear maps, attention, input stage + head); the backward is twice that"""
    d, ff, S = arch.latent_dim, arch.ff_size, T + 3
    lin = 2.0 * B * S * arch.num_layers * (3 * d * d + d * d + 2 * d * ff)
    att = 2.0 * B * arch.num_layers * 2 * S * S * d
    io = 2.0 * B * (T * (arch.input_dim + arch.obj_input_dim + arch.h2o_dim + 3 * d + d + arch.input_dim) * d + (arch.hand_shape_dim + arch.obj_embed_dim) * d)
    return lin, att, io


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--nobj", type=int, default=2)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--seconds", type=float, default=1.0)  # (a window of a fraction of a second measures the scheduler)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from oakink2_tamf_amd.model.segment_refine_model import SegmentRefineModel
    from oakink2_tamf_amd.model.segment_refine_train import SegmentRefineTrainStep

    if not torch.cuda.is_available():
        raise SystemExit("tools/refinetrain_bench.py measures on the GPU: no device visible")
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "config", "arch_refine.yml")) as f:
        cfg = yaml.safe_load(f)["model"]
    arch = R.mo.Arch(kind="R", **{k: int(cfg[k]) for k in R.ARCH_NAMES if k in cfg})
    sd = R.seeded_state_dict(arch, 1)
    inp, _ = R.seeded_inputs(arch, a.batch, a.frames, a.nobj, 2)
    batch = {k: torch.from_numpy(inp[k]).to(dev) for k in ("sample_pose_repr", "h2o_dist", "shape", "obj_embedding", "obj_traj")}
    batch["hand_side"] = inp["hand_side"]
    G = torch.from_numpy(np.random.default_rng(3).normal(size=inp["sample_pose_repr"].shape).astype(np.float32)).to(dev)

    model = SegmentRefineModel(**R.arch_dict(arch), dropout=a.dropout, precision="f32").to(dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    step = SegmentRefineTrainStep(model, a.batch, a.frames, dropout=a.dropout)
    n = [0]

    def hip():
        n[0] += 1
        out = step.forward(batch, step=n[0])
        out.backward(G)

    ref = TorchRefiner(arch, a.dropout).to(dev).train()
    side = torch.stack([torch.from_numpy(sd["hand_side_process.lh_embed" if s == "lh" else "hand_side_process.rh_embed"]) for s in inp["hand_side"]]).to(dev)
    pe = torch.from_numpy(sd["sequence_pos_encoder.pe"]).to(dev)

    def torch_step():
        for p in ref.parameters():
            p.grad = None
        ref(side, pe, batch).backward(G)

    lin, att, io = step_flop(arch, a.batch, a.frames, a.nobj)
    res = {"batch": a.batch, "frames": a.frames, "nobj": a.nobj, "dropout": a.dropout, "seconds": a.seconds, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "forward_gflop": {"layer_linear": lin / 1e9, "attention": att / 1e9, "input_and_head": io / 1e9},
           "step_tflop": 3 * (lin + att + io) / 1e12}
    for name, fn in (("hip", hip), ("torch", torch_step), ("hip_again", hip)):
        med, lo, hi, calls = timed(fn, a.seconds, a.warmup)
        res[name + "_ms"], res[name + "_ms_p10"], res[name + "_ms_p90"], res[name + "_calls"] = med, lo, hi, calls
    res["torch_over_hip"] = res["torch_ms"] / res["hip_ms"]
    res["hip_tflops"] = res["step_tflop"] / (res["hip_ms"] * 1e-3)
    # the breakdown, in a window of its own (the events cost host time): ms per step and launches per step of every kind of kernel
    step.profile(True)
    calls = 5
    for _ in range(calls):
        hip()
    prof = step.read_profile()
    step.profile(False)
    res["hip_kernels_ms_per_step"] = {k: v[1] / calls for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])}
    res["hip_kernels_launches_per_step"] = {k: v[0] // calls for k, v in prof.items()}
    res["hip_kernels_ms_sum"] = sum(v[1] for v in prof.values()) / calls
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")
    step.close()


if __name__ == "__main__":
    main()
