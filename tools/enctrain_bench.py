"""ms per training step (forward + loss + gradients of one batch) of the SegmentEncoder HIP training step beside a torch.nn assembly
of the same model doing forward + backward through PyTorch-ROCm autograd in fp32 on the same device, in the same run: config/arch_encoder.yml,
B = 256 clips of T = 160 frames, dropout 0.1, seeded weights and inputs.  HIP events around each of `--iters` calls after `--warmup`;
the median and the 10th / 90th percentiles are reported.  The optimiser is left out of both (it is the same PyTorch code on either side).

    python tools/enctrain_bench.py [--batch 256] [--frames 160] [--nobj 3] [--iters 300] [--warmup 20] [--json out.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")]
from encoder_restatement import ARCH_ENCODER, seeded_inputs, seeded_state_dict  # noqa: E402


class TorchEncoder(nn.Module):
    """the SegmentEncoder's training forward assembled from torch.nn modules (the state dict's key set)"""

    def __init__(self, arch, dropout):
        super().__init__()
        d = arch["latent_dim"]
        self.shape_embed, self.obj_embed = nn.Linear(arch["hand_shape_dim"], d), nn.Linear(arch["obj_embed_dim"], d)
        self.pose, self.traj = nn.Linear(arch["input_dim"], d), nn.Linear(arch["obj_input_dim"], d)
        self.merge = nn.Sequential(nn.Linear(2 * d, d), nn.SiLU(), nn.Linear(d, d))
        layer = nn.TransformerEncoderLayer(d_model=d, nhead=arch["num_heads"], dim_feedforward=arch["ff_size"], dropout=dropout, activation="gelu")
        self.enc = nn.TransformerEncoder(layer, num_layers=arch["num_layers"], enable_nested_tensor=False)
        self.head = nn.Sequential(nn.Linear(d, d), nn.SiLU(), nn.Linear(d, d), nn.SiLU(), nn.Linear(d, arch["input_dim"]))
        self.drop = nn.Dropout(dropout)

    def forward(self, side, cls, pe, b):
        prefix = torch.nan_to_num(torch.stack([side, self.shape_embed(b["shape"].mean(1)), self.obj_embed(b["obj_embedding"].mean(1))], 0))
        x = self.merge(torch.cat([self.pose(b["pose_repr"]), self.traj(b["obj_traj"]).mean(1)], -1))
        x = torch.nan_to_num(x).permute(1, 0, 2)
        seq = torch.cat([prefix, x, cls.expand(1, x.shape[1], -1)], 0)
        seq = self.drop(seq + pe[: seq.shape[0]])
        return self.head(self.enc(seq)[-1])


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
    return float(np.median(ms)), float(np.percentile(ms, 10)), float(np.percentile(ms, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--nobj", type=int, default=3)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=300)  # (about 1.5 s per side: a window of a fraction of a second measures the scheduler)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from oakink2_tamf_amd.model.segment_encoder import SegmentEncoder
    from oakink2_tamf_amd.model.segment_encoder_train import SegmentEncoderTrainStep

    dev = torch.device("cuda:0")
    arch = dict(ARCH_ENCODER)
    sd = seeded_state_dict(arch, 1)
    inp = seeded_inputs(a.batch, a.frames, a.nobj, 2)
    batch = {k: torch.from_numpy(inp[k]).to(dev) for k in ("pose_repr", "shape", "obj_embedding", "obj_traj")}
    batch["hand_side"] = inp["hand_side"]
    labels = torch.from_numpy(np.random.default_rng(3).integers(0, arch["input_dim"], a.batch)).to(dev)

    model = SegmentEncoder(69, **arch).to(dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    step = SegmentEncoderTrainStep(model, a.batch, a.frames, dropout=a.dropout)
    labels_np = labels.cpu().numpy()
    n = [0]

    def hip():
        n[0] += 1
        return step.loss_and_grads(batch, labels_np, step=n[0])["loss"]

    ref = TorchEncoder(arch, a.dropout).to(dev).train()
    side = torch.stack([torch.from_numpy(sd["hand_side_process.lh_embed" if s == "lh" else "hand_side_process.rh_embed"]) for s in inp["hand_side"]]).to(dev)
    cls = torch.from_numpy(sd["classification_token"]).to(dev)
    pe = torch.from_numpy(sd["sequence_pos_encoder.pe"]).to(dev)

    def torch_step():
        for p in ref.parameters():
            p.grad = None
        loss = nn.functional.cross_entropy(ref(side, cls, pe, batch), labels)
        loss.backward()
        return loss

    res = {"batch": a.batch, "frames": a.frames, "nobj": a.nobj, "dropout": a.dropout, "iters": a.iters, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    for name, fn in (("hip", hip), ("torch", torch_step), ("hip_again", hip)):  # (HIP before and after: drift of the box shows as a difference)
        med, lo, hi = timed(fn, a.iters, a.warmup)
        res[name + "_ms"], res[name + "_ms_p10"], res[name + "_ms_p90"] = med, lo, hi
    res["torch_over_hip"] = res["torch_ms"] / res["hip_ms"]
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")
    step.close()


if __name__ == "__main__":
    main()
