"""GPU: model/reconstruction_loss.HandReconstructionLoss on differentiable HIP MANO layers against the reference's own float64 run
(tests/golden/recloss_*.npz, tools/capture_recloss_golden.py).  Tolerance: measured, not chosen - every loss term and the gradient
with respect to the model output must lie within 4 x e32_* of the reference's float64 value, where e32_* is the deviation of the
REFERENCE's float32 run from its float64 run, stored in the fixture (absolute; the largest element for a gradient).
The module reduces its terms in float64, so what is measured here is the rounding of the HIP layer and of the float32 decode."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import mano_fixture as F  # noqa: E402
from test_recloss_cpu import coefs, refine_batch, scalar, segment_batch  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REF = {}


def _crit(fix):
    from oakink2_tamf_amd.mano import HipManoLayer, ManoArrays
    from oakink2_tamf_amd.model.reconstruction_loss import HandReconstructionLoss

    if "crit" not in _REF:
        layers = [HipManoLayer(ManoArrays(**F.synthetic_arrays(778, int(fix[k]))), center_idx=0, device=DEV, differentiable=True)
                  for k in ("seed_rh", "seed_lh")]
        _REF["crit"] = HandReconstructionLoss(layers[0], layers[1], fix["vpe"], fix["v_weights"], **coefs(fix)).to(DEV)
    return _REF["crit"]


def test_segment_loss_and_gradient_against_the_reference():
    fix = load_golden("recloss_segment.npz")
    crit = _crit(fix)
    out, batch = segment_batch(fix, torch.float32, DEV)
    out.requires_grad_(True)
    loss, d = crit(out, batch)
    loss.backward()
    assert loss.is_cuda and out.grad.dtype == torch.float32
    rows = []
    for k in ("loss", "rec_joint", "rec_vert", "edge_len"):
        rows.append((k, abs(scalar(d[k]) - float(fix[k])), float(fix["e32_" + k])))
    rows.append(("grad", float(np.abs(out.grad.cpu().double().numpy() - fix["grad"]).max()), float(fix["e32_grad"])))
    for k, err, e32 in rows:
        print(f"RECLOSS segment {k}: hip {err:.3e}  reference e32 {e32:.3e}  gate {4 * e32:.3e}")
    for k, err, e32 in rows:
        assert e32 > 0 and np.isfinite(err) and err <= 4 * e32, (k, err, e32)
    assert float(out.grad[1, :, :, 7:].abs().max()) == 0.0 and float(out.grad[2, :, :, 1:].abs().max()) == 0.0


def test_refine_terms_against_the_reference():
    fix = load_golden("recloss_refine.npz")
    crit = _crit(fix)
    out, batch = refine_batch(fix, torch.float32, DEV)
    loss, d = crit.refine_terms(out, batch)
    loss.backward()
    rows = [(k, abs(scalar(d[k]) - float(fix[k])), float(fix["e32_" + k])) for k in ("loss", "rec_joint", "rec_vert")]
    rows.append(("grad_joints", float(np.abs(out["refine_hand_joints"].grad.cpu().double().numpy() - fix["grad_joints"]).max()),
                 float(fix["e32_grad_joints"])))
    gv = out["refine_hand_verts"].grad.cpu().double().numpy()[:, :, ::int(fix["vert_stride"])]
    rows.append(("grad_verts", float(np.abs(gv - fix["grad_verts"]).max()), float(fix["e32_grad_verts"])))
    for k, err, e32 in rows:
        print(f"RECLOSS refine {k}: hip {err:.3e}  reference e32 {e32:.3e}  gate {4 * e32:.3e}")
    for k, err, e32 in rows:
        assert e32 > 0 and np.isfinite(err) and err <= 4 * e32, (k, err, e32)


def test_decode_agrees_with_the_hip_pose_decode():
    """the torch decode autograd carries against geometry.pose_repr_to_quat (tamf_pose_decode) on the fixture's pose rows: the gate of
    that kernel's own test (tests/test_geometry.py), q and -q being the same rotation when w == 0"""
    from oakink2_tamf_amd import geometry
    from oakink2_tamf_amd.model.reconstruction_loss import decode_pose_repr

    fix = load_golden("recloss_segment.npz")
    p = torch.from_numpy(fix["pose_repr"]).to(DEV)
    tsl, quat = decode_pose_repr(p)
    tsl_k, quat_k = geometry.pose_repr_to_quat(p)
    assert torch.equal(tsl, tsl_k) and quat.shape == quat_k.shape == (3, 12, 16, 4)
    q, r = quat.cpu().numpy(), quat_k.cpu().numpy()
    err = np.minimum(np.abs(q - r).max(-1), np.abs(q + r).max(-1) + (np.abs(r[..., 0]) > 1e-6) * 1e9)
    assert err.max() < 2e-6, err.max()
