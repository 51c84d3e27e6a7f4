"""CPU: the contact-distance terms of model/interaction_loss.HandInteractionLoss on the float64 restatements of the MANO layer
(tests/mano_restatement.py) and of the nearest-neighbour distances (tests/contact_restatement.py, injected as `contact_fn`) against the
reference's own float64 run of InteractionSegmentExtraLoss / SegmentRefineModelLoss with the distance terms on
(tests/golden/contact_loss_*.npz, written by tools/capture_contact_golden.py).  Both sides run float64 over the same formula, so the
bound is the tight one of tests/test_recloss_cpu.py.  Also here: the library's description in _lib, its export list against the C
header and the built file, and the Python-side refusals.  The kernels' part is tests/test_contact_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import contact_restatement as CS  # noqa: E402
import mano_fixture as F  # noqa: E402
import mano_restatement as R  # noqa: E402
from test_host_mirror import _declared, _nm_tamf  # noqa: E402
from test_recloss_cpu import SIDE, TIGHT, refine_batch, scalar, segment_batch  # noqa: E402

from oakink2_tamf_amd.mano import ManoArrays  # noqa: E402

SEG_KEYS = ("loss", "rec_joint", "rec_vert", "edge_len", "dist_h", "dist_o")
COEF_KEYS = ("coef_rec_joint_loss", "coef_rec_vert_loss", "coef_edge_len_loss", "coef_dist_h_loss", "coef_dist_o_loss")


def coefs(fix):
    return {k: float(fix[k]) for k in COEF_KEYS}


def contact_batch(fix, dtype, device="cpu"):
    out, batch = segment_batch(fix, dtype, device)
    for k in ("obj_traj", "obj_points"):
        batch[k] = torch.from_numpy(fix[k]).to(device=device, dtype=dtype)
    batch["obj_num"] = [int(n) for n in fix["obj_num"]]
    return out, batch


def contact_refine_batch(fix, dtype, device="cpu"):
    """the seeded tensors of tools/capture_contact_golden.py:refine_inputs (regenerated, not stored)"""
    B, T = fix["mask"].shape
    rng = np.random.default_rng(5400 + int(fix["refine_seed"]))
    tv, tj = 0.1 * rng.normal(size=(B, T, 778, 3)), 0.1 * rng.normal(size=(B, T, 21, 3))
    rv, rj = tv + 0.01 * rng.normal(size=tv.shape), tj + 0.01 * rng.normal(size=tj.shape)
    th = rng.uniform(0.0, 0.1, size=(B, T, 778))
    rh = np.abs(th + 0.01 * rng.normal(size=th.shape))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device=device, dtype=dtype)  # noqa: E731
    out = {"refine_hand_verts": t(rv).requires_grad_(True), "refine_hand_joints": t(rj).requires_grad_(True), "target_hand_verts": t(tv),
           "target_hand_joints": t(tj), "refine_h2o_dist": t(rh).requires_grad_(True), "target_h2o_dist": t(th)}
    return out, {"mask": torch.from_numpy(fix["mask"]).to(device=device, dtype=dtype)}


def _layers64(fix):
    return [R.TorchManoLayer(ManoArrays(**F.synthetic_arrays(778, int(fix[k]))), 0, "cpu", torch.float64) for k in ("seed_rh", "seed_lh")]


def _loss64(fix, **kw):
    from oakink2_tamf_amd.model.interaction_loss import HandInteractionLoss

    layers = _layers64(fix)
    return HandInteractionLoss(layers[0], layers[1], fix["vpe"], fix["v_weights"], **{**coefs(fix), **kw}, contact_fn=CS.signed_contact_distance,
                               normals_fn=CS.vertex_normals)


def test_fixture_is_the_shape_the_capture_tool_promises():
    fix = load_golden("contact_loss_segment.npz")
    assert [SIDE[int(s)] for s in fix["hand_side"]] == ["rh", "lh", "rh"] and fix["mask"].sum(1).tolist() == [6, 4, 1]
    assert fix["obj_num"].tolist() == [2, 1, 2] and fix["obj_points"].shape == (3, 2, 96, 3) and fix["obj_traj"].shape == (3, 2, 6, 9)
    assert coefs(fix)["coef_dist_h_loss"] == 0.1 and coefs(fix)["coef_dist_o_loss"] == 1.0 and fix["v_weights"].dtype == np.float32
    assert float(fix["cond_gap"]) >= 1e-5 and float(fix["cond_cos"]) >= 1e-4 and float(fix["cond_margin"]) >= 1e-5
    assert float(fix["cond_min_abs_pred"]) >= 1e-5 and int(fix["cond_min_class"]) >= 10 and bool(fix["cond_same"])
    assert float(fix["dist_h"]) > 0 and float(fix["dist_o"]) > 0
    assert not np.allclose(fix["obj_traj"][0, 0, 0], fix["obj_traj"][0, 0, 1])  # per-frame, non-identity poses
    assert np.abs(CS.rot6d_rows(torch.from_numpy(fix["obj_traj"][0, 0, :, 3:])).numpy() - np.eye(3)).max() > 0.1


def test_restated_terms_match_the_reference_in_float64():
    """the restatement alone: MANO restatement -> vertex normals -> dist_terms"""
    from oakink2_tamf_amd.model.reconstruction_loss import decode_pose_repr

    fix = load_golden("contact_loss_segment.npz")
    out, batch = contact_batch(fix, torch.float64)
    layers = dict(zip(("rh", "lh"), _layers64(fix)))
    pred = out.squeeze(2).permute(0, 2, 1)
    vp, vg, np_, ng = [], [], [], []
    for b, side in enumerate(batch["hand_side"]):
        for src, vs, ns in ((pred[b], vp, np_), (batch["pose_repr"][b], vg, ng)):
            tsl, quat = decode_pose_repr(src)
            verts = layers[side](pose_coeffs=quat, betas=batch["shape"][b]).verts + tsl[:, None]
            vs.append(verts), ns.append(CS.vertex_normals(verts, layers[side].th_faces))
    vw2 = torch.pow(torch.from_numpy(fix["v_weights"]), 1.0 / 2.5).double()
    dist_h, dist_o = CS.dist_terms(torch.stack(vp), torch.stack(np_), torch.stack(vg), torch.stack(ng), batch["obj_traj"], batch["obj_points"],
                                   batch["obj_num"], batch["mask"], vw2)
    for k, v in (("dist_h", dist_h), ("dist_o", dist_o)):
        assert abs(float(v) - float(fix[k])) <= TIGHT * abs(float(fix[k])), k


def test_interaction_loss_matches_the_reference_in_float64():
    fix = load_golden("contact_loss_segment.npz")
    crit = _loss64(fix)
    out, batch = contact_batch(fix, torch.float64)
    out.requires_grad_(True)
    loss, d = crit(out, batch)
    loss.backward()
    assert set(d) == set(SEG_KEYS) and scalar(d["dist_h"]) > 0 and scalar(d["dist_o"]) > 0
    for k in SEG_KEYS:
        assert abs(scalar(d[k]) - float(fix[k])) <= TIGHT * abs(float(fix[k])), (k, scalar(d[k]), float(fix[k]))
    assert scalar(d["loss"]) == scalar(loss) and loss.dtype == torch.float64
    g = fix["grad"]
    assert out.grad.shape == g.shape and np.abs(out.grad.numpy() - g).max() <= TIGHT * np.abs(g).max()
    # frames past a clip's mask get no gradient
    assert float(out.grad[1, :, :, 4:].abs().max()) == 0.0 and float(out.grad[2, :, :, 1:].abs().max()) == 0.0
    # the distance terms reach the gradient: without them it is another one
    crit0 = _loss64(fix, coef_dist_h_loss=0.0, coef_dist_o_loss=0.0)
    out0, _ = contact_batch(fix, torch.float64)
    out0.requires_grad_(True)
    loss0, d0 = crit0(out0, {k: v for k, v in batch.items() if not k.startswith("obj_")})  # (no object keys needed with the terms off)
    loss0.backward()
    assert d0["dist_h"] == 0.0 and d0["dist_o"] == 0.0 and float((out0.grad - out.grad).abs().max()) > 1e-3 * np.abs(g).max()


def test_each_distance_term_alone():
    fix = load_golden("contact_loss_segment.npz")
    out, batch = contact_batch(fix, torch.float64)
    for on, off in (("dist_h", "dist_o"), ("dist_o", "dist_h")):
        crit = _loss64(fix, **{f"coef_{off}_loss": 0.0})
        loss, d = crit(out, batch)
        assert d[off] == 0.0 and abs(scalar(d[on]) - float(fix[on])) <= TIGHT * float(fix[on])
        want = float(fix["loss"]) - float(fix[f"coef_{off}_loss"]) * float(fix[off])
        assert abs(scalar(loss) - want) <= 4 * TIGHT * float(fix["loss"])


def test_refine_terms_with_dist_h_match_the_reference_in_float64():
    fix = load_golden("contact_loss_refine.npz")
    crit = _loss64(fix)
    out, batch = contact_refine_batch(fix, torch.float64)
    loss, d = crit.refine_terms(out, batch)
    loss.backward()
    assert set(d) == {"loss", "rec_joint", "rec_vert", "dist_h"} and scalar(d["dist_h"]) > 0
    for k in ("loss", "rec_joint", "rec_vert", "dist_h"):
        assert abs(scalar(d[k]) - float(fix[k])) <= TIGHT * abs(float(fix[k])), k
    assert abs(float(CS.refine_dist_h(out["refine_h2o_dist"].detach(), out["target_h2o_dist"], batch["mask"], crit.v_weights2.double()))
               - float(fix["dist_h"])) <= TIGHT * float(fix["dist_h"])
    for key, name in (("grad_joints", "refine_hand_joints"), ("grad_h2o", "refine_h2o_dist")):
        assert np.abs(out[name].grad.numpy() - fix[key]).max() <= TIGHT * np.abs(fix[key]).max(), key
    gv = fix["grad_verts"]
    assert np.abs(out["refine_hand_verts"].grad.numpy()[:, :, ::int(fix["vert_stride"])] - gv).max() <= TIGHT * np.abs(gv).max()


def test_reconstruction_loss_is_unchanged_by_the_refactoring():
    """HandReconstructionLoss on recloss_*.npz: the reference's float64 terms as before, and the subclass with the distance terms off
    gives the same bits"""
    from oakink2_tamf_amd.model.interaction_loss import HandInteractionLoss
    from oakink2_tamf_amd.model.reconstruction_loss import HandReconstructionLoss

    fix = load_golden("recloss_segment.npz")
    layers = _layers64(fix)
    kw = {k: float(fix[k]) for k in COEF_KEYS[:3]}
    res = []
    for cls in (HandReconstructionLoss, HandInteractionLoss):
        crit = cls(layers[0], layers[1], fix["vpe"], fix["v_weights"].astype(np.float64), **kw)
        out, batch = segment_batch(fix, torch.float64)
        out.requires_grad_(True)
        loss, d = crit(out, batch)
        loss.backward()
        res.append((d, out.grad))
    (d, g), (d2, g2) = res
    for k in ("loss", "rec_joint", "rec_vert", "edge_len"):
        assert abs(scalar(d[k]) - float(fix[k])) <= TIGHT * abs(float(fix[k])), k
        assert scalar(d[k]) == scalar(d2[k])
    assert np.abs(g.numpy() - fix["grad"]).max() <= TIGHT * np.abs(fix["grad"]).max() and torch.equal(g, g2)
    assert d["dist_h"] == 0.0 and d["dist_o"] == 0.0 and d2["dist_h"] == 0.0 and d2["dist_o"] == 0.0
    with pytest.raises(NotImplementedError):  # the base class keeps its refusal
        HandReconstructionLoss(None, None, fix["vpe"], fix["v_weights"], 1.0, 1.0, coef_dist_h_loss=0.1)
    with pytest.raises(ValueError, match="negative"):
        HandInteractionLoss(None, None, fix["vpe"], fix["v_weights"], 1.0, 1.0, coef_dist_o_loss=-1.0)


def test_merged_h2o_dist_is_the_minimum_over_the_real_objects():
    from oakink2_tamf_amd.contact import merged_h2o_dist

    g = torch.Generator().manual_seed(3)
    hv = torch.randn(2, 3, 17, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    traj, pts = torch.randn(2, 3, 3, 9, generator=g, dtype=torch.float64), torch.randn(2, 3, 11, 3, generator=g, dtype=torch.float64)
    got = merged_h2o_dist(hv, traj, pts, [2, 3], contact_fn=CS.signed_contact_distance)
    want = CS.merged_h2o_dist(hv, traj, pts, [2, 3])
    assert got.shape == (2, 3, 17) and torch.allclose(got, want, rtol=1e-14, atol=0)
    got.sum().backward()
    assert torch.isfinite(hv.grad).all() and float(hv.grad.abs().max()) > 0


def test_library_description_and_exports():
    from oakink2_tamf_amd import _lib

    assert _lib.TRAINING == (_lib.ENCTRAIN, _lib.CONTACT)
    assert _lib.LIBRARIES == (_lib.SAMPLER, _lib.EVAL, _lib.MANO) and _lib.PREPROCESSING == (_lib.POINTENC,) and _lib.TEXT_PREPROCESSING == (_lib.TEXTENC,)
    assert len(_lib.EXPORTS) == 27 and len(_lib.EVAL_EXPORTS) == 4
    lib = _lib.CONTACT
    assert lib.root == "tamf_contact.hip" and lib.paths == [_lib.CONTACT_LIB_PATH] and lib.headers == ("tamf_contact.h", "tamf_hip.h")
    assert lib.sources == ["tamf_contact.h", "tamf_contact.hip", "tamf_device.h", "tamf_geom.h", "tamf_mesh.h"]
    assert len(lib.kernels) == 3 and not lib.counted_waits
    declared = _declared("tamf_contact.h")
    assert declared == set(_lib.CONTACT_EXPORTS) == set(lib.outputs[0].exports) and len(set(_lib.CONTACT_EXPORTS)) == len(_lib.CONTACT_EXPORTS)
    assert all(s.startswith("tamf_contact_") for s in _lib.CONTACT_EXPORTS)
    others = [_lib.EXPORTS, _lib.HOOK_EXPORTS, _lib.EVAL_EXPORTS, _lib.MANO_EXPORTS, _lib.POINTENC_EXPORTS, _lib.TEXTENC_EXPORTS, _lib.ENCTRAIN_EXPORTS]
    assert not set(_lib.CONTACT_EXPORTS) & set().union(*others)
    every = [l for group in (_lib.LIBRARIES, _lib.PREPROCESSING, _lib.TEXT_PREPROCESSING, _lib.TRAINING) for l in group]
    assert len({l.stamp_path for l in every}) == len(every) == 7
    lib.build()
    assert _nm_tamf(lib.paths[0]) == set(_lib.CONTACT_EXPORTS)
    assert not lib.stale()


def test_python_side_refusals():
    from oakink2_tamf_amd.contact import check_shapes

    hv, nrm, tr, pts = torch.zeros(2, 3, 5, 3), torch.zeros(2, 3, 5, 3), torch.zeros(2, 4, 3, 9), torch.zeros(2, 4, 7, 3)
    assert check_shapes(hv, nrm, tr, pts, None) == (2, 3, 5, 4, 7, None)
    assert check_shapes(hv, None, tr, pts, torch.tensor([1, 4]))[-1] == [1, 4]
    for bad in ([0, 1], [1, 5], [-1, 2]):
        with pytest.raises(ValueError, match=r"obj_num\[\d\] = -?\d+ of clip \d is outside \[1, nobj = 4\]"):
            check_shapes(hv, nrm, tr, pts, bad)
    with pytest.raises(ValueError, match="obj_num: expected 2 counts"):
        check_shapes(hv, nrm, tr, pts, [1, 2, 3])
    with pytest.raises(ValueError, match="hand_verts"):
        check_shapes(hv[..., :2], nrm, tr, pts, None)
    with pytest.raises(ValueError, match="hand_normals"):
        check_shapes(hv, nrm[:, :, :4], tr, pts, None)
    with pytest.raises(ValueError, match="obj_traj"):
        check_shapes(hv, nrm, tr[:, :, :2], pts, None)
    with pytest.raises(ValueError, match="obj_traj"):
        check_shapes(hv, nrm, tr[:, :3], pts, None)
    with pytest.raises(ValueError, match="obj_points"):
        check_shapes(hv, nrm, tr, pts[:1], None)
    # the loss refuses a batch whose object arrays do not fit it, before any layer call's result is used
    fix = load_golden("contact_loss_segment.npz")
    crit = _loss64(fix)
    out, batch = contact_batch(fix, torch.float64)
    with pytest.raises(ValueError, match="obj_num"):
        crit(out, dict(batch, obj_num=[2, 1]))
    with pytest.raises(ValueError, match="obj_traj / obj_points"):
        crit(out, dict(batch, obj_points=batch["obj_points"][:2]))
    with pytest.raises(ValueError, match="outside"):
        check_shapes(torch.zeros(3, 6, 778, 3), None, batch["obj_traj"], batch["obj_points"], [3, 1, 2])
