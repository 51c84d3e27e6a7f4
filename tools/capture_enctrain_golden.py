"""Capture the SegmentEncoder training fixtures (tests/golden/enctrain_*.npz, the perturbation adaptor's arrays and the action list)
from the reference.

Run where a checkout of the reference is available (CPU only):  python tools/capture_enctrain_golden.py REFERENCE_ROOT

The reference's own SegmentEncoder (model/segment_encoder.py) and SegmentEncoderLoss (model/segment_encoder_loss.py) are imported as
they are (tools/capture_encoder_golden.py's stubs for what they import but do not use) and run in train() mode with dropout 0.0, in
float64 and in float32.  A fixture holds seeded weights and inputs, labels, obj_num, the float64 loss, every gradient as the float32
rounding of its float64 value, and the measured gates (the weights themselves in the smallest case; elsewhere
the seed they are regenerated from and their SHA-256, to stay under the size limit of a committed file):
    tol_rel      = 4 * max over tensors of |g32 - g64|_inf / |g64|_inf     (the reference's own float32 run against its float64 run)
    tol_rel_loss = 4 * |loss32 - loss64| / |loss64|
The factor 4 is for a different but equally valid fp32 summation order over the B * S rows.  With a ragged obj_num the reference is
run one clip at a time on the clip's own objects (as its FID script does) and the loss is the mean over clips.
The SGD fixture adds 10 plain-SGD steps (lr 1e-2) of the reference on one batch: the float64 loss curve and the float32 run's largest
deviation from it.  Data only: no program text of the reference is stored.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oakink2-tamf_amd"))
import capture_encoder_golden as ceg  # noqa: E402
from encoder_restatement import ARCH_ENCODER, seeded_inputs, seeded_state_dict  # noqa: E402
from encoder_train_restatement import ARCH_NAMES, BUFFERS, sd_digest  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PE_ROWS = 256


def build(SegmentEncoder, arch, sd, dtype):
    model = SegmentEncoder(17, dropout=0.0, **{k: arch[k] for k in ARCH_NAMES}).train()
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not missing and not unexpected
    return model.to(dtype)


def batch_of(inputs, labels, dtype, rows=None, nobj=None):
    sl = slice(None) if rows is None else rows
    b = {k: torch.from_numpy(inputs[k][sl]).to(dtype) for k in ("pose_repr", "shape", "obj_embedding", "obj_traj")}
    if nobj is not None:
        b["obj_embedding"], b["obj_traj"] = b["obj_embedding"][:, :nobj], b["obj_traj"][:, :nobj]
    b["hand_side"] = list(inputs["hand_side"][sl]) if rows is not None else list(inputs["hand_side"])
    b["action_label_id"] = torch.from_numpy(np.asarray(labels)[sl]).long()
    return b


def loss_of(model, Loss, inputs, labels, obj_num, dtype):
    crit = Loss()
    if obj_num is None:
        batch = batch_of(inputs, labels, dtype)
        return crit(model(batch), batch)[0]
    total = 0.0
    for b, n in enumerate(obj_num):
        batch = batch_of(inputs, labels, dtype, rows=slice(b, b + 1), nobj=int(n))
        total = total + crit(model(batch), batch)[0]
    return total / len(obj_num)


def grads_of(SegmentEncoder, Loss, arch, sd, inputs, labels, obj_num, dtype):
    model = build(SegmentEncoder, arch, sd, dtype)
    loss = loss_of(model, Loss, inputs, labels, obj_num, dtype)
    loss.backward()
    g = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).double().numpy() for k, p in model.named_parameters()}
    assert not set(g) & set(BUFFERS)
    return float(loss.detach()), g


def sgd_curve(SegmentEncoder, Loss, arch, sd, inputs, labels, dtype, steps=10, lr=1e-2):
    model = build(SegmentEncoder, arch, sd, dtype)
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    out = []
    for _ in range(steps):
        opt.zero_grad()
        loss = loss_of(model, Loss, inputs, labels, None, dtype)
        loss.backward()
        opt.step()
        out.append(float(loss.detach()))
    return np.array(out, np.float64)


def capture(SegmentEncoder, Loss, name, arch, sd_seed, in_seed, B, T, nobj, obj_num=None, store_weights=True, sgd=False, nonfinite=False):
    sd = seeded_state_dict(arch, sd_seed)
    inp = seeded_inputs(B, T, nobj, seed=in_seed, obj_num=obj_num, arch=arch)
    inp["hand_side"] = ["rh" if b % 2 == 0 else "lh" for b in range(B)]
    if nonfinite:
        inp["pose_repr"][0, 1, 4] = np.inf
        inp["obj_traj"][B - 1, 0, 2:4, 1] = np.nan
        inp["obj_embedding"][0, 0, 3] = np.nan
    F = arch["input_dim"]
    labels = np.random.default_rng(in_seed + 1).integers(0, F, size=B).astype(np.int64)
    labels[0], labels[-1] = 0, F - 1
    if B == 1:
        labels[0] = F - 1
    l64, g64 = grads_of(SegmentEncoder, Loss, arch, sd, inp, labels, obj_num, torch.float64)
    l32, g32 = grads_of(SegmentEncoder, Loss, arch, sd, inp, labels, obj_num, torch.float32)
    # (non-finite inputs make whole gradient tensors NaN in torch - 0 * NaN in the weight gradients behind the nan_to_num mask: the
    #  pattern has to agree between the two runs, the gate is measured on the finite entries)
    assert all((np.isnan(g32[k]) == np.isnan(g64[k])).all() for k in g64)
    rel = max(np.nanmax(np.abs(g32[k] - g64[k])) / np.nanmax(np.abs(g64[k])) for k in g64 if not np.isnan(g64[k]).all() and np.nanmax(np.abs(g64[k])) > 0)
    data = {"arch": np.array([arch[k] for k in ARCH_NAMES], np.int32), "pe_head": sd["sequence_pos_encoder.pe"][:PE_ROWS, 0],
            "labels": labels, "loss": np.float64(l64), "tol_rel": np.float64(4 * rel), "tol_rel_loss": np.float64(4 * abs(l32 - l64) / abs(l64))}
    if store_weights:
        data.update({f"sd/{k}": v for k, v in sd.items() if k != "sequence_pos_encoder.pe"})
    else:
        data["sd_seed"] = np.int64(sd_seed)
        data["sd_sha256"] = np.array(sd_digest({k: v for k, v in sd.items() if k != "sequence_pos_encoder.pe"}))
    for k in ("pose_repr", "shape", "obj_embedding", "obj_traj"):
        data[f"in/{k}"] = inp[k]
    data["in/hand_side"] = np.array(inp["hand_side"])
    if obj_num is not None:
        data["in/obj_num"] = np.asarray(obj_num, np.int32)
    data.update({f"grad/{k}": v.astype(np.float32) for k, v in g64.items()})
    if sgd:
        c64 = sgd_curve(SegmentEncoder, Loss, arch, sd, inp, labels, torch.float64)
        c32 = sgd_curve(SegmentEncoder, Loss, arch, sd, inp, labels, torch.float32)
        data["sgd_loss"] = c64
        data["sgd_dev32"] = np.float64(np.abs(c32 - c64).max())
        data["sgd_lr"] = np.float64(1e-2)
    path = os.path.join(GOLDEN, name)
    np.savez_compressed(path, **data)
    print(f"{name}: loss {l64:.6f} tol_rel {4 * rel:.3e} tol_rel_loss {float(data['tol_rel_loss']):.3e}"
          + (f" sgd_dev32 {float(data['sgd_dev32']):.3e}" if sgd else "") + f" {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1000000


def capture_perturb(ref_root):
    """the reference's GuassianPerturbSampleAdaptor under a seeded np.random, and its action list"""
    from oakink2_tamf.dataset.action_adapter import ActionRecognitionAdapter
    from oakink2_tamf.dataset.pose_repr_sample import GuassianPerturbSampleAdaptor

    rng = np.random.default_rng(5)
    base = []
    for n, ln in ((20, 13), (20, 20), (20, 1)):
        pr = rng.normal(0, 0.5, (n, 99)).astype(np.float32)
        pr[ln:] = 0.0
        base.append({"pose_repr": pr, "len": ln})
    ad = GuassianPerturbSampleAdaptor([dict(b) for b in base], (0.01, 0.05))
    np.random.seed(1234)
    out = [ad[i] for i in range(len(base))]
    data = {"range": np.array([0.01, 0.05]), "seed": np.int64(1234)}
    for i, (b, o) in enumerate(zip(base, out)):
        data[f"pose_repr_{i}"], data[f"len_{i}"] = b["pose_repr"], np.int64(b["len"])
        data[f"sample_pose_repr_{i}"], data[f"sigma_{i}"] = o["sample_pose_repr"], np.float64(o["sample_info"][1])
    np.savez_compressed(os.path.join(GOLDEN, "enctrain_perturb.npz"), **data)
    with open(os.path.join(GOLDEN, "enctrain_action_list.txt"), "w") as f:
        f.write("\n".join(ActionRecognitionAdapter([]).action_list) + "\n")
    print("enctrain_perturb.npz, enctrain_action_list.txt")


def main(ref_root: str):
    SegmentEncoder, _ = ceg.import_reference(ref_root)
    from oakink2_tamf.model.segment_encoder_loss import SegmentEncoderLoss as Loss

    small = dict(ARCH_ENCODER, obj_embed_dim=32)
    capture(SegmentEncoder, Loss, "enctrain_small_ragged.npz", small, 101, 102, B=3, T=12, nobj=3, obj_num=[1, 3, 2], store_weights=False)
    capture(SegmentEncoder, Loss, "enctrain_l1_ff16.npz", dict(small, num_layers=1, ff_size=16), 111, 112, B=2, T=7, nobj=1)
    capture(SegmentEncoder, Loss, "enctrain_nonfinite.npz", dict(small, num_layers=3), 121, 122, B=3, T=28, nobj=2, nonfinite=True, store_weights=False)
    capture(SegmentEncoder, Loss, "enctrain_full_arch.npz", dict(ARCH_ENCODER), 131, 132, B=2, T=61, nobj=2, store_weights=False)
    capture(SegmentEncoder, Loss, "enctrain_sgd.npz", small, 141, 142, B=6, T=12, nobj=2, sgd=True, store_weights=False)
    capture_perturb(ref_root)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tools/capture_enctrain_golden.py REFERENCE_ROOT")
    main(sys.argv[1])
