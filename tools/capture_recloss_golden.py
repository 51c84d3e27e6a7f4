"""Capture the reconstruction-loss fixtures (tests/golden/recloss_*.npz) from the reference.

Run where a checkout of the reference is available (CPU only):  python tools/capture_recloss_golden.py REFERENCE_ROOT

The reference's own InteractionSegmentExtraLoss (coef_dist_* = 0) and SegmentRefineModelLoss (coef_dist_h = 0) are imported as they are
and run in float64 and in float32.  What they import but this package cannot ship is stood in for:
  manotorch.manolayer.ManoLayer   the float64 / float32 restatement tests/mano_restatement.TorchManoLayer on the seeded MANO-shaped
                                  arrays tests/mano_fixture.synthetic_arrays(778, seed) (right: seed 0, left: seed 1), centre 0
  pytorch3d.structures.Meshes     an inert stand-in: the reference computes the normals but does not use them with the distance terms off
The `vpe` file is the unique edges of the fixture's faces, the `c_weight` file seeded weights in [0, 1] (float32, as the reference
loads them).

recloss_segment.npz: 3 clips (rh, lh, rh), T = 12, mask lengths 12 / 7 / 1; the float32 inputs, the seeds of the arrays, vpe and
v_weights; the reference's float64 loss terms and d loss / d model_output; and per quantity e32_* = the deviation of the reference's
float32 run from its float64 run (absolute; the largest element for the gradient).
recloss_refine.npz: the same for SegmentRefineModelLoss on seeded refine_* / target_* tensors (regenerated from the seed by
`refine_inputs`, not stored); the gradient with respect to refine_hand_joints whole, with respect to refine_hand_verts at every
16th vertex.
Data only: no program text of the reference is stored, and no MANO array."""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oakink2-tamf_amd"))
import mano_fixture as MF  # noqa: E402
import mano_restatement as MR  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEEDS = {"right": 0, "left": 1}
B, T, V, MASK_LEN, SIDES = 3, 12, 778, (12, 7, 1), ("rh", "lh", "rh")
COEF = dict(coef_rec_joint_loss=1.0, coef_rec_vert_loss=1.0, coef_edge_len_loss=0.1)  # the reference's config/loss_param*.yml
VERT_STRIDE = 16
_dtype = [torch.float64]  # what the stand-in layers compute in (set per run)


def unique_edges(faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    return np.unique(np.sort(e, axis=1), axis=0).astype(np.int64)


def segment_inputs(seed=0):
    """float32 arrays: model_output (B, 99, 1, T), pose_repr (B, T, 99), shape (B, T, 10), mask (B, T)"""
    rng = np.random.default_rng(4200 + seed)
    gt = rng.normal(size=(B, T, 99))
    gt[..., :3] *= 0.1
    pred = gt + 0.2 * rng.normal(size=gt.shape)
    shape = np.repeat(rng.normal(size=(B, 1, 10)), T, axis=1)
    mask = np.stack([(np.arange(T) < n).astype(np.float64) for n in MASK_LEN])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    return f32(pred.transpose(0, 2, 1)[:, :, None, :]), f32(gt), f32(shape), f32(mask)


def refine_inputs(seed=0):
    """float32 arrays: refine / target verts (B, T, V, 3) and joints (B, T, 21, 3), hand-sized"""
    rng = np.random.default_rng(4300 + seed)
    tv, tj = 0.1 * rng.normal(size=(B, T, V, 3)), 0.1 * rng.normal(size=(B, T, 21, 3))
    rv, rj = tv + 0.01 * rng.normal(size=tv.shape), tj + 0.01 * rng.normal(size=tj.shape)
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (rv, rj, tv, tj))


def v_weights_of(seed=0):
    return np.random.default_rng(4400 + seed).random(V).astype(np.float32)


def install_stand_ins():
    from oakink2_tamf_amd.mano import ManoArrays

    class ManoLayer:
        def __init__(self, mano_assets_root=None, rot_mode=None, side=None, center_idx=None, use_pca=None, flat_hand_mean=None):
            assert rot_mode == "quat" and center_idx == 0 and use_pca is False and flat_hand_mean is True
            self.arrays = ManoArrays(**MF.synthetic_arrays(V, SEEDS[side]))
            self.th_faces = torch.as_tensor(self.arrays.faces).long()

        def __call__(self, pose_coeffs, betas):
            return MR.TorchManoLayer(self.arrays, 0, "cpu", _dtype[0])(pose_coeffs, betas)

    class Meshes:
        def __init__(self, verts, faces):
            self.verts = verts

        def verts_normals_packed(self):
            return torch.zeros(self.verts.shape[0] * self.verts.shape[1], 3, dtype=self.verts.dtype)

    mt, ml = types.ModuleType("manotorch"), types.ModuleType("manotorch.manolayer")
    ml.ManoLayer, mt.manolayer = ManoLayer, ml
    p3, ps = types.ModuleType("pytorch3d"), types.ModuleType("pytorch3d.structures")
    ps.Meshes, p3.structures = Meshes, ps
    sys.modules.update({"manotorch": mt, "manotorch.manolayer": ml, "pytorch3d": p3, "pytorch3d.structures": ps})


def run_segment(Loss, cfg, arrays, dtype):
    _dtype[0] = dtype
    crit = Loss("unused", cfg).to(dtype)
    out, gt, shape, mask = (torch.from_numpy(a).to(dtype) for a in arrays)
    out.requires_grad_(True)
    batch = {"hand_side": list(SIDES), "shape": shape, "obj_list": [[]] * B, "obj_verts": [[]] * B, "obj_traj": [None] * B, "mask": mask,
             "pose_repr": gt}
    loss, d = crit(out, batch)
    loss.backward()
    res = {k: float(d[k]) for k in ("loss", "rec_joint", "rec_vert", "edge_len")}
    res["grad"] = out.grad.double().numpy()
    return res


def run_refine(Loss, cfg, arrays, mask, dtype):
    crit = Loss(cfg).to(dtype)
    rv, rj, tv, tj = (torch.from_numpy(a).to(dtype) for a in arrays)
    rv.requires_grad_(True), rj.requires_grad_(True)
    loss, d = crit({"refine_hand_verts": rv, "refine_hand_joints": rj, "target_hand_verts": tv, "target_hand_joints": tj},
                   {"mask": torch.from_numpy(mask).to(dtype)})
    loss.backward()
    res = {k: float(d[k]) for k in ("loss", "rec_joint", "rec_vert")}
    res["grad_joints"], res["grad_verts"] = rj.grad.double().numpy(), rv.grad.double().numpy()[:, :, ::VERT_STRIDE]
    return res


def with_e32(r64, r32):
    out = {}
    for k, v in r64.items():
        out[k] = np.asarray(v, dtype=np.float64)
        out["e32_" + k] = np.float64(np.abs(np.asarray(r32[k]) - np.asarray(v)).max())
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    install_stand_ins()
    sys.path.insert(0, os.path.join(sys.argv[1], "src"))
    from oakink2_tamf.model.interaction_segment_extra_loss import InteractionSegmentExtraLoss
    from oakink2_tamf.model.segment_refine_model_loss import SegmentRefineModelLoss

    vpe = unique_edges(MF.synthetic_arrays(V, 0)["faces"])
    vw = v_weights_of()
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "vpe.npy"), vpe)
        np.save(os.path.join(tmp, "w.npy"), vw)
        cfg = dict(COEF, coef_dist_h_loss=0.0, coef_dist_o_loss=0.0, vpe_path=os.path.join(tmp, "vpe.npy"), c_weight_path=os.path.join(tmp, "w.npy"))
        seg = segment_inputs()
        s64, s32 = (run_segment(InteractionSegmentExtraLoss, cfg, seg, dt) for dt in (torch.float64, torch.float32))
        ref = refine_inputs()
        r64, r32 = (run_refine(SegmentRefineModelLoss, cfg, ref, seg[3], dt) for dt in (torch.float64, torch.float32))
    common = dict(vpe=vpe.astype(np.int32), v_weights=vw, mask=seg[3], hand_side=np.array([0 if s == "rh" else 1 for s in SIDES], np.int32),
                  seed_rh=np.int32(SEEDS["right"]), seed_lh=np.int32(SEEDS["left"]), **{k: np.float64(v) for k, v in COEF.items()})
    np.savez_compressed(os.path.join(GOLDEN, "recloss_segment.npz"), model_output=seg[0], pose_repr=seg[1], shape=seg[2], **common,
                        **with_e32(s64, s32))
    np.savez_compressed(os.path.join(GOLDEN, "recloss_refine.npz"), refine_seed=np.int32(0), vert_stride=np.int32(VERT_STRIDE), **common,
                        **with_e32(r64, r32))
    for name, r in (("segment", with_e32(s64, s32)), ("refine", with_e32(r64, r32))):
        print(name, {k: (float(v) if np.ndim(v) == 0 else f"max |.| {np.abs(v).max():.3e}") for k, v in r.items()})


if __name__ == "__main__":
    main()
