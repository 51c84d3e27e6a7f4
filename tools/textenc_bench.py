"""ms for a batch of prompts through the native text encoder (libtamf_textenc.so, full ViT-B/32 size, seeded weights) beside the
float32 torch.nn assembly of the same model (tests/textenc_restatement.torch_tower) on the same device in the same run.  Every
prompt has `--tokens` ids (EOT at the last of them; the reference's call allows 22).  The torch assembly is timed twice: on the
same `--tokens` positions, and on the full 77-position context as the reference's call runs it.  HIP events around `--iters` calls
after `--warmup`; the median is reported.

    python tools/textenc_bench.py [--prompts 256] [--tokens 22] [--iters 10] [--warmup 3] [--json out.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")]
import textenc_restatement as R  # noqa: E402


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
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, default=256)
    ap.add_argument("--tokens", type=int, default=22)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from oakink2_tamf_amd.model.text_encoder import HipClipTextEncoder

    dev = torch.device("cuda:0")
    cfg = R.CONFIGS["full"]
    sd = R.seeded_state_dict(cfg, R.WEIGHT_SEED["full"])
    ids = R.seeded_ids(cfg, [a.tokens - 1] * a.prompts, 5)
    enc = HipClipTextEncoder(cfg, device=dev)
    enc.load_state_dict(sd)
    tower = R.torch_tower(sd, cfg, torch.float32, dev)
    short = ids[:, : a.tokens].copy()
    res = {"prompts": a.prompts, "tokens": a.tokens, "rows": int(a.prompts * a.tokens), "iters": a.iters}
    with torch.no_grad():
        for name, fn in (("hip", lambda: enc.encode_tokens(ids)), ("torch_f32_same_rows", lambda: tower(short)), ("torch_f32_full_context", lambda: tower(ids))):
            res[name + "_ms"], res[name + "_ms_min"], res[name + "_ms_max"] = timed(fn, a.iters, a.warmup)
        out, ref = enc.encode_tokens(ids), tower(ids)
        res["max_abs_diff_hip_vs_torch_f32"] = float((out - ref).abs().max())
    enc.close()
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
