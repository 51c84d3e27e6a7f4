"""CPU: model/reconstruction_loss.py on the float64 restatement of the MANO layer (tests/mano_restatement.TorchManoLayer) against the
reference's own float64 run of InteractionSegmentExtraLoss / SegmentRefineModelLoss (tests/golden/recloss_*.npz, written by
tools/capture_recloss_golden.py).  Both sides run float64 over the same formula, so the bound is tight: 64 * eps64 * the size of the
reference value (|value|, or max |grad| for a gradient).  This pins the pose decode, the masks, the means and the batching by hand
side; the HIP layer's part is tests/test_recloss_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import mano_fixture as F  # noqa: E402
import mano_restatement as R  # noqa: E402

from oakink2_tamf_amd.mano import ManoArrays  # noqa: E402
from oakink2_tamf_amd.model import reconstruction_loss as RL  # noqa: E402

TIGHT = 64 * float(np.finfo(np.float64).eps)
SIDE = {0: "rh", 1: "lh"}


def scalar(x):
    return float(x.detach()) if torch.is_tensor(x) else float(x)


def coefs(fix):
    return {k: float(fix[k]) for k in ("coef_rec_joint_loss", "coef_rec_vert_loss", "coef_edge_len_loss")}


def segment_batch(fix, dtype, device="cpu"):
    t = lambda k: torch.from_numpy(fix[k]).to(device=device, dtype=dtype)  # noqa: E731
    return t("model_output"), {"hand_side": [SIDE[int(s)] for s in fix["hand_side"]], "shape": t("shape"), "mask": t("mask"), "pose_repr": t("pose_repr")}


def refine_batch(fix, dtype, device="cpu"):
    """the seeded refine_* / target_* tensors of tools/capture_recloss_golden.py:refine_inputs (regenerated, not stored)"""
    B, T = fix["mask"].shape
    rng = np.random.default_rng(4300 + int(fix["refine_seed"]))
    tv, tj = 0.1 * rng.normal(size=(B, T, 778, 3)), 0.1 * rng.normal(size=(B, T, 21, 3))
    rv, rj = tv + 0.01 * rng.normal(size=tv.shape), tj + 0.01 * rng.normal(size=tj.shape)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device=device, dtype=dtype)  # noqa: E731
    out = {"refine_hand_verts": t(rv).requires_grad_(True), "refine_hand_joints": t(rj).requires_grad_(True), "target_hand_verts": t(tv),
           "target_hand_joints": t(tj)}
    return out, {"mask": torch.from_numpy(fix["mask"]).to(device=device, dtype=dtype)}


def _loss64(fix):
    layers = [R.TorchManoLayer(ManoArrays(**F.synthetic_arrays(778, int(fix[k]))), 0, "cpu", torch.float64) for k in ("seed_rh", "seed_lh")]
    return RL.HandReconstructionLoss(layers[0], layers[1], fix["vpe"], fix["v_weights"].astype(np.float64), **coefs(fix))


def test_segment_loss_matches_the_reference_in_float64():
    fix = load_golden("recloss_segment.npz")
    assert [SIDE[int(s)] for s in fix["hand_side"]] == ["rh", "lh", "rh"] and fix["mask"].sum(1).tolist() == [12, 7, 1]
    crit = _loss64(fix)
    out, batch = segment_batch(fix, torch.float64)
    out.requires_grad_(True)
    loss, d = crit(out, batch)
    loss.backward()
    assert set(d) == {"loss", "rec_joint", "rec_vert", "edge_len", "dist_h", "dist_o"} and d["dist_h"] == 0.0 and d["dist_o"] == 0.0
    for k in ("loss", "rec_joint", "rec_vert", "edge_len"):
        assert abs(scalar(d[k]) - float(fix[k])) <= TIGHT * abs(float(fix[k])), k
    assert scalar(d["loss"]) == scalar(loss)
    g = fix["grad"]
    assert out.grad.shape == g.shape and np.abs(out.grad.numpy() - g).max() <= TIGHT * np.abs(g).max()
    # frames past a clip's mask get no gradient
    assert float(out.grad[1, :, :, 7:].abs().max()) == 0.0 and float(out.grad[2, :, :, 1:].abs().max()) == 0.0


def test_disabled_terms_are_plain_zeros():
    fix = load_golden("recloss_segment.npz")
    crit = _loss64(fix)
    crit.coef_rec_vert_loss = crit.coef_edge_len_loss = 0.0
    out, batch = segment_batch(fix, torch.float64)
    loss, d = crit(out, batch)
    assert d["rec_vert"] == 0.0 and d["edge_len"] == 0.0 and abs(scalar(loss) - float(fix["rec_joint"])) <= TIGHT * float(fix["rec_joint"])


def test_refine_terms_match_the_reference_in_float64():
    fix = load_golden("recloss_refine.npz")
    crit = _loss64(fix)
    out, batch = refine_batch(fix, torch.float64)
    loss, d = crit.refine_terms(out, batch)
    loss.backward()
    assert set(d) == {"loss", "rec_joint", "rec_vert", "dist_h"} and d["dist_h"] == 0.0
    for k in ("loss", "rec_joint", "rec_vert"):
        assert abs(scalar(d[k]) - float(fix[k])) <= TIGHT * abs(float(fix[k])), k
    gj, gv = fix["grad_joints"], fix["grad_verts"]
    assert np.abs(out["refine_hand_joints"].grad.numpy() - gj).max() <= TIGHT * np.abs(gj).max()
    assert np.abs(out["refine_hand_verts"].grad.numpy()[:, :, ::int(fix["vert_stride"])] - gv).max() <= TIGHT * np.abs(gv).max()


def test_decode_against_the_reference_quaternions():
    """tests/golden/geometry.npz holds the reference's quaternions of 64 pose rows (float32): the gate of the HIP decode's own test"""
    fix = load_golden("geometry.npz")
    tsl, quat = RL.decode_pose_repr(torch.from_numpy(fix["pose"]))
    np.testing.assert_array_equal(tsl.numpy(), fix["pose"][:, :3])
    q, r = quat.numpy(), fix["quat"]
    # rows 1-4 are exact 180-degree rotations / degenerate inputs: q and -q describe the same rotation when w == 0
    err = np.minimum(np.abs(q - r).max(-1), np.abs(q + r).max(-1) + (np.abs(r[..., 0]) > 1e-6) * 1e9)
    assert err.max() < 2e-6, err.max()
    # through the rotation matrices, in float64: the quaternion describes the matrix Gram-Schmidt gave
    p = torch.from_numpy(fix["pose"]).double()
    _, q64 = RL.decode_pose_repr(p)
    rot = RL.rot6d_to_rotmat(p[:, 3:].reshape(-1, 16, 6))
    ok = (rot.det() - 1).abs() < 1e-9  # (the degenerate rows give no rotation)
    assert int(ok.sum()) > 0.9 * ok.numel()
    assert float((R.quat_to_rotmat(q64)[ok] - rot[ok]).abs().max()) < 1e-12
    assert float(q64[..., 0].min()) >= 0.0
    # batched shape, and autograd reaches the input
    p3 = p.reshape(4, 16, 99).clone().requires_grad_(True)
    t3, q3 = RL.decode_pose_repr(p3)
    assert t3.shape == (4, 16, 3) and q3.shape == (4, 16, 16, 4) and torch.equal(q3.reshape(64, 16, 4), q64)
    q3.sum().backward()
    assert torch.isfinite(p3.grad).all() and float(p3.grad[..., 3:].abs().max()) > 0 and float(p3.grad[..., :3].abs().max()) == 0


def test_distance_terms_are_refused_and_an_empty_mask_raises():
    fix = load_golden("recloss_segment.npz")
    for k in ("coef_dist_h_loss", "coef_dist_o_loss"):
        with pytest.raises(NotImplementedError, match="nearest-neighbour distance.*vertex normals"):
            RL.HandReconstructionLoss(None, None, fix["vpe"], fix["v_weights"], 1.0, 1.0, 0.1, **{k: 0.5})
    with pytest.raises(ValueError, match="vpe"):
        RL.HandReconstructionLoss(None, None, np.array([[0, 778]]), fix["v_weights"], 1.0, 1.0)
    crit = _loss64(fix)
    out, batch = segment_batch(fix, torch.float64)
    batch["mask"][1] = 0
    with pytest.raises(ValueError, match="no valid frame"):
        crit(out, batch)
    with pytest.raises(ValueError, match="no valid frame"):
        crit.refine_terms(refine_batch(load_golden("recloss_refine.npz"), torch.float64)[0], {"mask": batch["mask"]})
    with pytest.raises(ValueError, match="hand_side"):
        crit(out, dict(batch, hand_side=["rh", "lh", "xh"]))
