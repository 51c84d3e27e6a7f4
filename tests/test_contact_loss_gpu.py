"""GPU: model/interaction_loss.HandInteractionLoss on differentiable HIP MANO layers, the HIP vertex normals and the HIP contact-distance
kernels against the reference's own float64 run with the distance terms on (tests/golden/contact_loss_*.npz,
tools/capture_contact_golden.py).  Tolerance: measured, not chosen - the rule of tests/test_recloss_gpu.py: every loss term and the
gradient must lie within 4 x e32_* of the reference's float64 value, where e32_* is the deviation of the REFERENCE's float32 run from
its float64 run, stored in the fixture.  The fixture's inputs keep every index, sign and weight class away from where float32
rounding could flip it (the capture tool asserts that), so no element is left out of any comparison."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import mano_fixture as F  # noqa: E402
from test_contact_cpu import SEG_KEYS, coefs, contact_batch, contact_refine_batch  # noqa: E402
from test_recloss_cpu import scalar  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REF = {}


def _crit(fix):
    from oakink2_tamf_amd.mano import HipManoLayer, ManoArrays
    from oakink2_tamf_amd.model.interaction_loss import HandInteractionLoss

    if "crit" not in _REF:
        layers = [HipManoLayer(ManoArrays(**F.synthetic_arrays(778, int(fix[k]))), center_idx=0, device=DEV, differentiable=True)
                  for k in ("seed_rh", "seed_lh")]
        _REF["crit"] = HandInteractionLoss(layers[0], layers[1], fix["vpe"], fix["v_weights"], **coefs(fix)).to(DEV)
    return _REF["crit"]


def test_segment_loss_with_distance_terms_against_the_reference():
    fix = load_golden("contact_loss_segment.npz")
    crit = _crit(fix)
    out, batch = contact_batch(fix, torch.float32, DEV)
    out.requires_grad_(True)
    loss, d = crit(out, batch)
    loss.backward()
    assert loss.is_cuda and out.grad.dtype == torch.float32 and scalar(d["dist_h"]) > 0 and scalar(d["dist_o"]) > 0
    rows = [(k, abs(scalar(d[k]) - float(fix[k])), float(fix["e32_" + k])) for k in SEG_KEYS]
    rows.append(("grad", float(np.abs(out.grad.cpu().double().numpy() - fix["grad"]).max()), float(fix["e32_grad"])))
    for k, err, e32 in rows:
        print(f"RECLOSS contact segment {k}: hip {err:.3e}  reference e32 {e32:.3e}  gate {4 * e32:.3e}")
    for k, err, e32 in rows:
        assert e32 > 0 and np.isfinite(err) and err <= 4 * e32, (k, err, e32)
    assert float(out.grad[1, :, :, 4:].abs().max()) == 0.0 and float(out.grad[2, :, :, 1:].abs().max()) == 0.0


def test_refine_terms_with_dist_h_against_the_reference():
    fix = load_golden("contact_loss_refine.npz")
    crit = _crit(fix)
    out, batch = contact_refine_batch(fix, torch.float32, DEV)
    loss, d = crit.refine_terms(out, batch)
    loss.backward()
    rows = [(k, abs(scalar(d[k]) - float(fix[k])), float(fix["e32_" + k])) for k in ("loss", "rec_joint", "rec_vert", "dist_h")]
    for key, name in (("grad_joints", "refine_hand_joints"), ("grad_h2o", "refine_h2o_dist")):
        rows.append((key, float(np.abs(out[name].grad.cpu().double().numpy() - fix[key]).max()), float(fix["e32_" + key])))
    gv = out["refine_hand_verts"].grad.cpu().double().numpy()[:, :, ::int(fix["vert_stride"])]
    rows.append(("grad_verts", float(np.abs(gv - fix["grad_verts"]).max()), float(fix["e32_grad_verts"])))
    for k, err, e32 in rows:
        print(f"RECLOSS contact refine {k}: hip {err:.3e}  reference e32 {e32:.3e}  gate {4 * e32:.3e}")
    for k, err, e32 in rows:
        assert e32 > 0 and np.isfinite(err) and err <= 4 * e32, (k, err, e32)
