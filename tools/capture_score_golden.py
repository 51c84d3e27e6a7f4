#!/usr/bin/env python
"""Capture the PSKL-J fixtures of tests/golden/ from the reference's own arithmetic.  CPU, numpy only.

    python tools/capture_score_golden.py REFERENCE_ROOT [--out tests/golden]

The PSKL-J arithmetic is inline in the `main()` of REFERENCE_ROOT/script/compute_score/compute_score_psklj.py.  This tool reads that
script when it runs, cuts the block that starts at the line `dataset_psd_list = []` and ends with the line `print(pskl_1, pskl_2)` -
found by content, not by line number - and executes it on the `dataset_res_list` / `model_res_list` it supplies (synthetic joints with
the reference's tail hold applied, as :270-271 does before the lists are filled).  Only arrays are stored: the inputs, the reference's
`dataset_psd`, `model_psd`, `pskl_1`, `pskl_2`, and the numpy version that produced them.  Nothing of the reference's text is written.

Fixtures: psklj_t160.npz (smooth clips vs the same family with jitter, T = 160, random len in [40, 160]), psklj_t7.npz (T = 7, L = 5),
psklj_degenerate.npz with two cases under the prefixes `const/` (the dataset constant in time: all its spectra 0, the 1e-8 alone
decides) and `same/` (both sets identical: both scores 0).  The Contact-Ratio distance is already pinned by tests/golden/contact.npz."""
import argparse
import contextlib
import io
import os
import textwrap

import numpy as np

START, END = "dataset_psd_list = []", "print(pskl_1, pskl_2)"


def reference_block(reference_root: str) -> str:
    path = os.path.join(reference_root, "script", "compute_score", "compute_score_psklj.py")
    with open(path) as f:
        lines = f.read().splitlines()
    first = [i for i, l in enumerate(lines) if l.strip() == START]
    last = [i for i, l in enumerate(lines) if l.strip() == END]
    if len(first) != 1 or len(last) != 1 or last[0] <= first[0]:
        raise SystemExit(f"{path}: the block from `{START}` to `{END}` was not found exactly once")
    return textwrap.dedent("\n".join(lines[first[0]: last[0] + 1]))


def run_reference(block: str, dataset_joints, model_joints, lens):
    """the reference's block on the two lists of (T, J, 3) float32 clips, tail hold applied first (:270-271)"""
    def held(x):
        out = []
        for clip, l in zip(x, lens):
            c = np.array(clip, dtype=np.float32, copy=True)
            c[int(l):, :, :] = c[int(l) - 1, :, :]
            out.append(c)
        return out

    scope = {"np": np, "dataset_res_list": held(dataset_joints), "model_res_list": held(model_joints)}
    with contextlib.redirect_stdout(io.StringIO()):
        exec(compile(block, "<reference psklj block>", "exec"), scope)
    return {"dataset_psd": np.asarray(scope["dataset_psd"]), "model_psd": np.asarray(scope["model_psd"]),
            "pskl_1": np.asarray(scope["pskl_1"]), "pskl_2": np.asarray(scope["pskl_2"])}


def smooth_clips(rng, n, T, J=21, n_modes=4, amp=0.05):
    """hand-like trajectories: a few low-frequency sinusoids per coordinate plus a slow drift, metres"""
    t = np.arange(T, dtype=np.float64)[None, :, None, None] / 30.0  # 30 fps
    x = rng.normal(scale=0.2, size=(n, 1, J, 3)) + rng.normal(scale=0.02, size=(n, 1, J, 3)) * t
    for _ in range(n_modes):
        freq = rng.uniform(0.2, 2.5, size=(n, 1, J, 3))
        x = x + amp * rng.uniform(0.2, 1.0, size=(n, 1, J, 3)) * np.sin(2 * np.pi * freq * t + rng.uniform(0, 2 * np.pi, size=(n, 1, J, 3)))
    return x.astype(np.float32)


def case(block, dataset_joints, model_joints, lens, prefix=""):
    ref = run_reference(block, dataset_joints, model_joints, lens)
    out = {"dataset_joints": dataset_joints, "model_joints": model_joints, "lens": np.asarray(lens, np.int32), **ref}
    return {prefix + k: v for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference_root")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    a = ap.parse_args()
    block = reference_block(a.reference_root)
    ver = np.asarray(np.__version__)
    os.makedirs(a.out, exist_ok=True)

    rng = np.random.default_rng(20260)
    n, T = 5, 160
    ds = smooth_clips(rng, n, T)
    md = smooth_clips(rng, n, T) + rng.normal(scale=2e-3, size=(n, T, 21, 3)).astype(np.float32)
    lens = rng.integers(40, T + 1, size=n)
    lens[0] = T
    np.savez_compressed(os.path.join(a.out, "psklj_t160.npz"), numpy_version=ver, **case(block, ds, md.astype(np.float32), lens))

    rng = np.random.default_rng(20261)
    n, T = 6, 7
    ds = smooth_clips(rng, n, T, amp=0.2)
    md = smooth_clips(rng, n, T, amp=0.2) + rng.normal(scale=5e-3, size=(n, T, 21, 3)).astype(np.float32)
    lens = np.array([7, 7, 6, 5, 4, 7])
    np.savez_compressed(os.path.join(a.out, "psklj_t7.npz"), numpy_version=ver, **case(block, ds, md.astype(np.float32), lens))

    rng = np.random.default_rng(20262)
    n, T = 3, 16
    moving = smooth_clips(rng, n, T, amp=0.2)
    const = np.broadcast_to(moving[:, :1], moving.shape).copy()
    lens = np.array([16, 12, 9])
    deg = {"numpy_version": ver}
    deg.update(case(block, const, moving, lens, "const/"))
    deg.update(case(block, moving, moving.copy(), lens, "same/"))
    np.savez_compressed(os.path.join(a.out, "psklj_degenerate.npz"), **deg)
    for name in ("psklj_t160.npz", "psklj_t7.npz", "psklj_degenerate.npz"):
        p = os.path.join(a.out, name)
        with np.load(p) as z:
            scores = {k: float(z[k]) for k in z.files if k.endswith(("pskl_1", "pskl_2"))}
            dt = {k: str(z[k].dtype) for k in z.files if k.endswith("_psd")}
        print(name, os.path.getsize(p), "bytes", scores, dt)


if __name__ == "__main__":
    main()
