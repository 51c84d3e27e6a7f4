"""GPU: the `pen` term of model/interaction_loss.HandInteractionLoss on differentiable HIP MANO layers and the HIP SDF-lattice sampler
against a float64 torch restatement of the same loss: tests/mano_restatement.py's layer, then tests/sdfgrid_restatement.depth_torch
injected as `pen_fn`, so that autograd gives the reference gradient.

Tolerance: measured, not chosen - the project's standing gate.  The loss value, the `pen` value and the gradient with respect to the
model output (its largest element) must lie within 4 x the error the SAME restatement makes when it runs in float32 against its
float64 run on the same inputs.  Both figures are printed before they are compared.

The scene: the synthetic MANO-shaped arrays and the batch of tests/golden/recloss_segment.npz (three clips, right, left, right); one
sphere lattice, its radius the distance from a fingertip vertex to its 40th nearest vertex, carried along with the PREDICTED hand's
fingertip frame by frame under a generic rotation, so the prediction's fingertip lies inside and the ground truth's mostly does not."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import mano_fixture as F  # noqa: E402
import mano_restatement as MR  # noqa: E402
import sdfgrid_cases as C  # noqa: E402
import sdfgrid_restatement as RS  # noqa: E402
from test_recloss_cpu import coefs, scalar, segment_batch  # noqa: E402

from oakink2_tamf_amd import sdfgrid  # noqa: E402
from oakink2_tamf_amd.mano import HipManoLayer, ManoArrays  # noqa: E402
from oakink2_tamf_amd.model.interaction_loss import HandInteractionLoss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIP, PEN = 745, 2.0  # the vertex the sphere follows; the coefficient
_S = {}


def restated_pen(packed, dtype):
    """depth_torch behind the pen_fn contract: (B, nobj, T, V), zero rows for padded objects and objects without a lattice"""

    def fn(hand_verts, obj_traj, grid_id, obj_num=None):
        rows = []
        for o in range(obj_traj.shape[1]):
            d = RS.depth_torch(packed[0], hand_verts, obj_traj[:, o], dtype)
            has = torch.as_tensor([int(g) == 0 and (obj_num is None or o < int(obj_num[b])) for b, g in enumerate(grid_id[:, o].tolist())])
            rows.append(d * has.to(d)[:, None, None])
        return torch.stack(rows, dim=1)

    return fn


def _layers(fix, dtype):
    return [MR.TorchManoLayer(ManoArrays(**F.synthetic_arrays(778, int(fix[k]))), 0, "cpu", dtype) for k in ("seed_rh", "seed_lh")]


def scene():
    """-> fix, the lattice's fields, obj_traj (3, 2, T, 9) float32 around the predicted fingertips, grid_id, obj_num"""
    if not _S:
        fix = load_golden("recloss_segment.npz")
        out, batch = segment_batch(fix, torch.float64)
        probe = HandInteractionLoss(*_layers(fix, torch.float64), fix["vpe"], fix["v_weights"], 1.0, 1.0)
        B, T = batch["mask"].shape
        tips, radius = np.zeros((B, T, 3)), None
        for _, idx, verts_p, *_ in probe._per_side(out, batch):
            v = verts_p.detach().numpy()
            tips[idx.numpy()] = v[:, :, TIP]
            if radius is None:
                radius = float(np.sort(np.linalg.norm(v[0, 0] - v[0, 0, TIP], axis=-1))[40])
        rng = np.random.default_rng(21)
        traj = np.zeros((B, 2, T, 9))
        traj[:, 0, :, :3] = tips + rng.normal(size=tips.shape) * 0.1 * radius
        traj[:, 1, :, :3] = tips + np.array([1.0, 0.0, 0.0])  # a second object 1 m away: never touched
        traj[..., 3:] = rng.normal(size=(B, 2, 1, 6))  # a generic rotation per clip and object, constant over the frames
        fields = C.fields_from(C.sphere_fn(radius), [0, 0, 0], [3 * radius] * 3, 24)
        _S.update(fix=fix, fields=fields, traj=traj.astype(np.float32), grid_id=torch.tensor([[0, 0], [0, -1], [0, 0]], dtype=torch.int32), obj_num=[2, 1, 2],
                  radius=radius)
    return _S


def _batch(dtype, device, far=False):
    s = scene()
    out, batch = segment_batch(s["fix"], dtype, device)
    traj = s["traj"].copy()
    if far:
        traj[..., 0] += 1.0  # the same hand, every object 1 m away
    batch.update(obj_traj=torch.from_numpy(traj).to(device=device, dtype=dtype), sdf_grid_id=s["grid_id"].to(device), obj_num=list(s["obj_num"]))
    return out, batch


def _reference(dtype, rec: bool, refine=None):
    """the restatement's loss dict and gradient in `dtype` on the CPU"""
    s = scene()
    fix, packed = s["fix"], [sdfgrid.pack_grid(s["fields"])]
    c = coefs(fix) if rec else {"coef_rec_joint_loss": 0.0, "coef_rec_vert_loss": 0.0}
    crit = HandInteractionLoss(*_layers(fix, dtype), fix["vpe"], fix["v_weights"].astype(np.float64 if dtype == torch.float64 else np.float32), **c,
                               coef_pen_loss=PEN, pen_fn=restated_pen(packed, dtype))
    out, batch = _batch(dtype, "cpu")
    if refine is None:
        out.requires_grad_(True)
        loss, d = crit(out, batch)
        loss.backward()
        return {k: scalar(v) for k, v in d.items()}, out.grad.double().numpy()
    return refine(crit, batch, dtype, "cpu")


def _hip_crit(rec: bool):
    s = scene()
    fix = s["fix"]
    key = ("crit", rec)
    if key not in _S:
        if "layers" not in _S:
            _S["layers"] = [HipManoLayer(ManoArrays(**F.synthetic_arrays(778, int(fix[k]))), center_idx=0, device=DEV, differentiable=True)
                            for k in ("seed_rh", "seed_lh")]
            _S["grids"] = sdfgrid.SdfGridSet([s["fields"]], device=DEV)
        c = coefs(fix) if rec else {"coef_rec_joint_loss": 0.0, "coef_rec_vert_loss": 0.0}
        _S[key] = HandInteractionLoss(*_S["layers"], fix["vpe"], fix["v_weights"], **c, coef_pen_loss=PEN, sdf_grids=_S["grids"]).to(DEV)
    return _S[key]


def _gate(name, rows):
    for k, err, e32 in rows:
        print(f"PENLOSS {name} {k}: hip {err:.3e}  restatement float32 {e32:.3e}  gate {4 * e32:.3e}")
    for k, err, e32 in rows:
        assert e32 > 0 and np.isfinite(err) and err <= 4 * e32, (name, k, err, e32)


@pytest.mark.parametrize("rec", [True, False], ids=["with_rec_terms", "pen_alone"])
def test_segment_loss_with_pen_inside_the_gate(rec):
    d64, g64 = _reference(torch.float64, rec)
    d32, g32 = _reference(torch.float32, rec)
    out, batch = _batch(torch.float32, DEV)
    out.requires_grad_(True)
    loss, d = _hip_crit(rec)(out, batch)
    loss.backward()
    assert loss.is_cuda and loss.dtype == torch.float64 and list(d)[-1] == "pen" and d64["pen"] > 0
    print(f"sphere radius {scene()['radius']:.4f}; pen {d64['pen']:.6e} of loss {d64['loss']:.6e}")
    rows = [(k, abs(scalar(d[k]) - d64[k]), abs(d32[k] - d64[k])) for k in ("loss", "pen")]
    rows.append(("grad", float(np.abs(out.grad.cpu().double().numpy() - g64).max()), float(np.abs(g32 - g64).max())))
    _gate("segment " + ("rec + pen" if rec else "pen alone"), rows)
    if not rec:
        assert float(np.abs(g64).max()) > 0 and float(out.grad.abs().max()) > 0  # fingertips inside: a gradient


def test_the_same_hand_a_metre_away_gives_exactly_zero_and_a_zero_gradient():
    out, batch = _batch(torch.float32, DEV, far=True)
    out.requires_grad_(True)
    loss, d = _hip_crit(False)(out, batch)
    loss.backward()
    assert scalar(d["pen"]) == 0.0 and scalar(loss) == 0.0 and (out.grad is None or not bool(out.grad.any()))


def test_a_prediction_equal_to_the_ground_truth_gives_zero():
    """e is an excess: however deep the ground truth lies, predicting it costs nothing"""
    out, batch = _batch(torch.float32, DEV)
    same = batch["pose_repr"].permute(0, 2, 1).unsqueeze(2).contiguous().requires_grad_(True)
    crit = _hip_crit(False)
    deepest = 0.0
    with torch.no_grad():  # carry the sphere with the ground truth's own fingertip, so that the ground truth does lie inside
        for _, idx, _, _, verts_g, _, _ in crit._per_side(same.detach(), batch):
            batch["obj_traj"][idx, 0, :, :3] = verts_g[:, :, TIP]
            deepest = max(deepest, float(_S["grids"].penetration_depth(verts_g, batch["obj_traj"][idx], batch["sdf_grid_id"][idx]).max()))
    assert deepest > 0
    loss, d = crit(same, batch)
    loss.backward()
    assert scalar(d["pen"]) == 0.0 and not bool(same.grad.any())


def _refine(crit, batch, dtype, device):
    """refine_terms through refine_step_loss with the refined pose as a leaf: -> (loss dict, gradient with respect to it)"""
    from oakink2_tamf_amd.model.segment_refine_train import refine_step_loss

    s = scene()
    pred = segment_batch(s["fix"], dtype, device)[0].squeeze(2).permute(0, 2, 1).contiguous().requires_grad_(True)  # (B, T, 99)
    B, T = batch["mask"].shape
    zeros = lambda hv, tr, pts, on: torch.zeros(hv.shape[:3], dtype=hv.dtype, device=hv.device)  # noqa: E731 (dist_h is off: the feature is not read)
    total, terms, res = refine_step_loss(lambda h: pred, batch, crit, torch.zeros(B, 2, 4, 3, dtype=dtype, device=device), batch["obj_num"],
                                         h2o_dist=torch.zeros(B, T, 778, dtype=dtype, device=device), merged_fn=zeros)
    total.backward()
    return {k: scalar(v) for k, v in terms.items()}, pred.grad.double().cpu().numpy()


def test_refine_terms_with_pen_through_refine_step_loss_inside_the_gate():
    d64, g64 = _reference(torch.float64, True, refine=_refine)
    d32, g32 = _reference(torch.float32, True, refine=_refine)
    _, batch = _batch(torch.float32, DEV)
    d, g = _refine(_hip_crit(True), batch, torch.float32, DEV)
    assert list(d)[-1] == "pen" and d64["pen"] > 0
    rows = [(k, abs(d[k] - d64[k]), abs(d32[k] - d64[k])) for k in ("loss", "pen")]
    rows.append(("grad", float(np.abs(g - g64).max()), float(np.abs(g32 - g64).max())))
    _gate("refine rec + pen", rows)
    # far away: exactly zero, and the loss is the reconstruction terms alone
    _, far = _batch(torch.float32, DEV, far=True)
    d_far, _ = _refine(_hip_crit(True), far, torch.float32, DEV)
    assert d_far["pen"] == 0.0
    # the refined pose equal to the ground truth: zero
    crit = _hip_crit(False)
    from oakink2_tamf_amd.model.segment_refine_train import refine_step_loss

    B, T = batch["mask"].shape
    zeros = lambda hv, tr, pts, on: torch.zeros(hv.shape[:3], dtype=hv.dtype, device=hv.device)  # noqa: E731
    _, terms, _ = refine_step_loss(lambda h: batch["pose_repr"].clone(), batch, crit, torch.zeros(B, 2, 4, 3, device=DEV), batch["obj_num"],
                                   h2o_dist=torch.zeros(B, T, 778, device=DEV), merged_fn=zeros)
    assert scalar(terms["pen"]) == 0.0
