"""SegmentRefineTrainStep.loss_and_grads on the MI355X against the reference's whole training step (tests/golden/refinetrain_e2e.npz:
its own SegmentRefineModel and SegmentRefineModelLoss): HIP trunk forward, pose decode, the native differentiable MANO layer built
from the same synthetic arrays, the HIP nearest neighbour, HandInteractionLoss.refine_terms, HIP trunk backward.  Loss terms, output
and every parameter gradient inside the fixture's gates (4 x the reference's own float32-against-float64 error)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mano_fixture as MF  # noqa: E402
import refine_train_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_loss_and_grads_against_the_reference():
    import torch

    from oakink2_tamf_amd.mano import HipManoLayer, ManoArrays
    from oakink2_tamf_amd.model.interaction_loss import HandInteractionLoss
    from oakink2_tamf_amd.model.segment_refine_model import SegmentRefineModel
    from oakink2_tamf_amd.model.segment_refine_train import SegmentRefineTrainStep

    c = R.load_case(os.path.join(HERE, "golden", "refinetrain_e2e.npz"))
    z, inp = c["z"], c["inputs"]
    layers = [HipManoLayer(ManoArrays(**MF.synthetic_arrays(778, int(z[k]))), center_idx=0, device=DEV, differentiable=True) for k in ("seed_rh", "seed_lh")]
    crit = HandInteractionLoss(layers[0], layers[1], np.zeros((0, 2), np.int64), z["v_weights"], float(z["coef_rec_joint_loss"]),
                               float(z["coef_rec_vert_loss"]), coef_dist_h_loss=float(z["coef_dist_h_loss"])).to(DEV)
    m = SegmentRefineModel(**R.arch_dict(c["arch"]), dropout=0.0, precision="f32").to(DEV)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in c["sd"].items()})
    B, T = inp["sample_pose_repr"].shape[:2]
    ts = SegmentRefineTrainStep(m, B, T, dropout=0.0)
    for p in m.parameters():
        p.grad.fill_(float("nan"))
    batch = {k: torch.from_numpy(inp[k]) for k in ("sample_pose_repr", "pose_repr", "shape", "obj_embedding", "obj_traj", "mask")}
    batch["hand_side"] = inp["hand_side"]
    res = ts.loss_and_grads(batch, crit, torch.from_numpy(inp["obj_points"]), obj_num=c["obj_num"])
    torch.cuda.synchronize()
    assert {"refine_pose_repr", "refine_hand_verts", "refine_hand_joints", "refine_h2o_dist", "target_hand_verts", "target_hand_joints",
            "target_h2o_dist", "sample_h2o_dist"} <= set(res["output"])
    tol_term = float(z["tol_rel_term"])
    for k in ("loss", "rec_joint", "rec_vert", "dist_h"):
        ref, got = float(z[f"term/{k}"]), float(res[k])
        print(f"{k}: {got:.9f} ref {ref:.9f} rel {abs(got - ref) / abs(ref):.3e} (gate {tol_term:.3e})")
        assert abs(got - ref) <= tol_term * abs(ref), k
    e_out = R.rel_err(res["output"]["refine_pose_repr"].cpu().numpy(), c["out"])
    err = R.fixture_grad_err({k: v.grad.cpu().numpy() for k, v in m.named_parameters()}, c)
    worst = max(err, key=err.get)
    print(f"output rel {e_out:.3e} (gate {c['tol_rel_out']:.3e}); worst gradient {worst} rel {err[worst]:.3e} (gate {c['tol_rel']:.3e})")
    assert e_out <= c["tol_rel_out"]
    assert err[worst] <= c["tol_rel"], (worst, err[worst])
    ts.close()
