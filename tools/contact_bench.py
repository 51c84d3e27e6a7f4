#!/usr/bin/env python
"""Times the contact-distance kernels (contact.signed_contact_distance: forward, and forward + backward) against the way the same
results are obtained without them: the torch restatement tests/contact_restatement.py on the same device - broadcast squared
distances (no cdist), `argmin`, gather, autograd - looped over clips, objects and chunks of frames as its memory needs
(frames x V x P x 3 floats per chunk).  Needs the GPU.

    python tools/contact_bench.py [--reps 5] [--out contact_bench.json]

  reduced    4 clips, 16 frames, 2 objects, 778 hand vertices, 2 048 points: both paths run the whole shape
  training   64 clips, 160 frames, 2 objects, 8 192 points (the reference's training shape): the kernels run the whole shape; the
             restatement runs ONE clip of it (2 objects, 160 frames) and its time is multiplied by 64 - it is a loop over the clips,
             so that is what the whole shape costs (`restatement_scaled_by` in the output)
Every figure: device events around a window of back-to-back calls, sized from a first call to last about 50 ms, after one warm-up call
of the same shape; `reps` windows per path, the paths alternating; the per-call median of the windows is reported with min and max.
Results are compared before they are timed: on the compared part at least 99.99 % of the indices must be equal and at least
99.99 % of the signs (random clouds are not kept away from float32 near-ties) and the distances within
1e-4 relative + 1e-6 m (two float32 evaluations of clouds a few decimetres wide)."""
import argparse
import json
import os
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)

from siv_bench import alternate, stats  # noqa: E402

CHUNK_FLOATS = 2 ** 27  # the restatement's (frames, V, P, 3) difference tensor per chunk: 512 MiB of float32


def inputs(B, T, nobj, V, P, seed=0):
    import torch

    import contact_restatement as CS

    g = torch.Generator().manual_seed(seed)
    hv = 0.1 * torch.randn(B, T, V, 3, generator=g)
    nrm = CS.unit(torch.randn(B, T, V, 3, generator=g))
    tr = torch.cat([0.05 * torch.randn(B, nobj, T, 3, generator=g), torch.randn(B, nobj, T, 6, generator=g)], dim=-1)
    pts = 0.1 * torch.randn(B, nobj, P, 3, generator=g)
    up = (torch.randn(B, nobj, T, P, generator=g), torch.randn(B, nobj, T, V, generator=g))
    return [t.cuda() for t in (hv, nrm, tr, pts)], [t.cuda() for t in up]


def restatement(hv, nrm, tr, pts, up=None):
    """the restatement over clips, objects and frame chunks -> (o2h, h2o, o2h_idx); with `up`, also backward into hv.grad"""
    import torch

    import contact_restatement as CS

    B, T, V, _ = hv.shape
    nobj, P = pts.shape[1], pts.shape[2]
    step = max(1, CHUNK_FLOATS // (V * P * 3))
    o2h, h2o, idx = (torch.empty(B, nobj, T, n, device=hv.device, dtype=dt) for n, dt in ((P, hv.dtype), (V, hv.dtype), (P, torch.int32)))
    for b in range(B):
        for o in range(nobj):
            for t0 in range(0, T, step):
                sl = slice(t0, min(T, t0 + step))
                moved = CS.move_points(tr[b, o, sl], pts[b, o])
                a, c, ai, _ = CS.point2point_signed(hv[b, sl], moved, nrm[b, sl])
                if up is not None:
                    ((a * up[0][b, o, sl]).sum() + (c * up[1][b, o, sl]).sum()).backward()
                o2h[b, o, sl], h2o[b, o, sl], idx[b, o, sl] = a.detach(), c.detach(), ai.to(torch.int32)
    return o2h, h2o, idx


def kernels(hv, nrm, tr, pts, up=None):
    from oakink2_tamf_amd import contact

    o2h, h2o, idx = contact.signed_contact_distance(hv, nrm, tr, pts)
    if up is not None:
        ((o2h * up[0]).sum() + (h2o * up[1]).sum()).backward()
    return o2h.detach(), h2o.detach(), idx


def run(name, dims, ref_clips, reps):
    import torch

    B, T, nobj, V, P = dims
    inp, up = inputs(*dims)
    sub, sub_up = [t[:ref_clips] for t in inp], [t[:ref_clips] for t in up]
    with torch.no_grad():
        got, want = kernels(*inp), restatement(*sub)
    same = float((got[2][:ref_clips] == want[2]).float().mean())
    assert same >= 0.9999, f"indices differ: {same}"
    ok = got[2][:ref_clips] == want[2]
    signs = float((got[0][:ref_clips].sign() == want[0].sign()).float().mean())
    assert signs >= 0.9999, f"signs differ: {signs}"
    assert torch.allclose(got[0][:ref_clips][ok].abs(), want[0][ok].abs(), rtol=1e-4, atol=1e-6) and torch.allclose(got[1][:ref_clips], want[1], rtol=1e-4, atol=1e-6)

    def leaf(ts):
        return [ts[0].detach().clone().requires_grad_(True)] + list(ts[1:])

    def fwd_k():
        with torch.no_grad():
            kernels(*inp)

    def fwd_r():
        with torch.no_grad():
            restatement(*sub)

    fb_k = lambda: kernels(*leaf(inp), up=up)  # noqa: E731
    fb_r = lambda: restatement(*leaf(sub), up=sub_up)  # noqa: E731
    (t_fk, t_fr, t_bk, t_br), calls = alternate((fwd_k, fwd_r, fb_k, fb_r), reps)
    scale = B / ref_clips
    row = {"shape": name, "B": B, "T": T, "nobj": nobj, "V": V, "P": P, "pairs_per_direction": B * T * nobj * V * P, "index_agreement": same, "sign_agreement": signs,
           "restatement_clips_timed": ref_clips, "restatement_scaled_by": scale, "calls_per_window": calls,
           "kernels_forward": stats(t_fk), "kernels_forward_backward": stats(t_bk),
           "restatement_forward": stats(t_fr), "restatement_forward_backward": stats(t_br)}
    row["speedup_forward"] = scale * row["restatement_forward"]["median_ms"] / row["kernels_forward"]["median_ms"]
    row["speedup_forward_backward"] = scale * row["restatement_forward_backward"]["median_ms"] / row["kernels_forward_backward"]["median_ms"]
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    res = {"device": torch.cuda.get_device_name(0), "rows": [run("reduced", (4, 16, 2, 778, 2048), 4, a.reps), run("training", (64, 160, 2, 778, 8192), 1, a.reps)]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
