"""InterationSegmentMDMTrainStep.loss_and_grads on the MI355X with a HandInteractionLoss as the callback (reconstruction and distance
terms on): q_sample, HIP forward of G, the masked MSE, pose decode, the native differentiable MANO layer built from the synthetic arrays
of tests/mano_fixture.py, the HIP nearest neighbour, HIP backward of G - against float64 autograd on the CPU through the restatement of
G and the same loss object on torch MANO layers and the torch nearest neighbour.  Tiny architecture at head dimension 128, B 2 (rh,
lh), T 5; the hands, objects and masks are the inputs of tests/golden/refinetrain_e2e.npz.

Gate: 4 x the error of the same CPU computation in float32 against float64, measured here and printed (terms: not below the rounding
of the one float32 each is returned as).  This pins the glue, not the loss, which has its own fixtures."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "oakink2-tamf_amd"))
import mano_fixture as MF  # noqa: E402
import mdm_train_restatement as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COEF = dict(coef_rec_joint_loss=1.0, coef_rec_vert_loss=1.0, coef_dist_h_loss=0.1, coef_dist_o_loss=1.0)  # the reference's config/loss_param.yml
TERMS = ("rec_joint", "rec_vert", "dist_h", "dist_o")


def _case():
    arch = M.ARCH_TINY_128
    z = np.load(os.path.join(HERE, "golden", "refinetrain_e2e.npz"), allow_pickle=False)
    inp = {k: z[f"in/{k}"] for k in ("pose_repr", "shape", "obj_embedding", "obj_traj", "mask", "obj_points")}
    inp["hand_side"], obj_num = [str(s) for s in z["in/hand_side"]], [int(n) for n in z["in/obj_num"]]
    B, T = inp["pose_repr"].shape[:2]
    assert (B, T, inp["hand_side"]) == (2, 5, ["rh", "lh"]) and inp["obj_embedding"].shape[2] == arch.obj_embed_dim
    rng = np.random.default_rng(9100)
    inp["text_embedding"] = rng.normal(size=(B, arch.clip_dim)).astype(np.float32)
    t, noise = np.array([37, 611], np.int64), rng.normal(size=(B, arch.input_dim, 1, T)).astype(np.float32)
    return arch, M.seeded_state_dict(arch, 9101), inp, obj_num, t, noise, z


def _batch(inp, obj_num, dtype, device):
    import torch

    b = {k: torch.from_numpy(np.ascontiguousarray(inp[k])).to(device=device, dtype=dtype)
         for k in ("pose_repr", "shape", "obj_embedding", "obj_traj", "obj_points", "text_embedding")}
    b["mask"], b["hand_side"], b["obj_num"] = torch.from_numpy(inp["mask"]).to(device), inp["hand_side"], obj_num
    return b


def _cpu_run(arch, sd_np, inp, obj_num, t, noise, z, diffusion, dtype):
    """the whole step on the CPU in `dtype` -> ({term: float}, {key: gradient float64})"""
    import torch

    import contact_restatement as CS
    import mano_restatement as MR
    from oakink2_tamf_amd.mano import ManoArrays
    from oakink2_tamf_amd.model.interaction_loss import HandInteractionLoss
    from oakink2_tamf_amd.model.interaction_segment_mdm_train import training_losses

    layers = []
    for key in ("seed_rh", "seed_lh"):
        arrays = ManoArrays(**MF.synthetic_arrays(778, int(z[key])))
        layer = MR.TorchManoLayer(arrays, 0, "cpu", dtype)
        layer.th_faces = torch.as_tensor(arrays.faces).long()
        layers.append(layer)
    crit = HandInteractionLoss(layers[0], layers[1], np.zeros((0, 2), np.int64), z["v_weights"], contact_fn=CS.signed_contact_distance,
                               normals_fn=CS.vertex_normals, **COEF)
    sd = M.leaf_state_dict(sd_np, dtype)
    batch = _batch(inp, obj_num, dtype, "cpu")

    def model(x_t, ts, batch):
        return M.mdm_train_forward(sd, arch, x_t, ts, batch, dtype, obj_num=obj_num)

    x_start = batch["pose_repr"].unsqueeze(3).permute(0, 2, 3, 1)
    terms, (extra, extra_dict) = training_losses(diffusion, model, x_start, torch.from_numpy(t), model_kwargs={"batch": batch},
                                                 noise=torch.from_numpy(noise).to(dtype), loss_callback=crit)
    diffusion_loss = terms["loss"].mean()
    total = diffusion_loss + extra
    total.backward()
    vals = {"loss": float(total.detach()), "diffusion_loss": float(diffusion_loss.detach()), **{k: float(extra_dict[k].detach()) for k in TERMS}}
    return vals, {k: v.grad.double().numpy() for k, v in sd.items() if k not in M.BUFFERS}


def test_loss_and_grads_against_float64_autograd():
    import torch

    from oakink2_tamf_amd.mano import HipManoLayer, ManoArrays
    from oakink2_tamf_amd.model.diffusion_util import create_gaussian_diffusion
    from oakink2_tamf_amd.model.interaction_loss import HandInteractionLoss
    from oakink2_tamf_amd.model.interaction_segment_mdm import InterationSegmentMDM
    from oakink2_tamf_amd.model.interaction_segment_mdm_train import InterationSegmentMDMTrainStep

    arch, sd, inp, obj_num, t, noise, z = _case()
    diffusion = create_gaussian_diffusion(1000, "cosine")
    v64, g64 = _cpu_run(arch, sd, inp, obj_num, t, noise, z, diffusion, torch.float64)
    v32, g32 = _cpu_run(arch, sd, inp, obj_num, t, noise, z, diffusion, torch.float32)
    assert all(v64[k] > 0 for k in v64)  # every term is on
    tol_term = {k: 4 * max(abs(v32[k] - v64[k]) / abs(v64[k]), 2.0 ** -24) for k in v64}
    tol = 4 * max(M.grad_rel_err(g32, g64).values())

    layers = [HipManoLayer(ManoArrays(**MF.synthetic_arrays(778, int(z[k]))), center_idx=0, device=DEV, differentiable=True) for k in ("seed_rh", "seed_lh")]
    crit = HandInteractionLoss(layers[0], layers[1], np.zeros((0, 2), np.int64), z["v_weights"], **COEF).to(DEV)
    m = InterationSegmentMDM(**M.arch_dict(arch), dropout=0.0, precision="f32").to(DEV)
    m.load_state_dict(M.module_state_dict(sd))
    ts = InterationSegmentMDMTrainStep(m, 2, 5, dropout=0.0)
    for p in m.parameters():
        p.grad.fill_(float("nan"))
    res = ts.loss_and_grads(diffusion, _batch(inp, obj_num, torch.float32, "cpu"), crit, t=torch.from_numpy(t), noise=torch.from_numpy(noise), obj_num=obj_num)
    torch.cuda.synchronize()
    got = {"loss": float(res["loss"]), "diffusion_loss": float(res["diffusion_loss"]), **{k: float(res["extra"][k]) for k in TERMS}}
    for k, ref in v64.items():
        print(f"{k}: {got[k]:.9f} ref {ref:.9f} rel {abs(got[k] - ref) / abs(ref):.3e} (gate {tol_term[k]:.3e})")
    err = M.grad_rel_err({k: v.grad.cpu().numpy() for k, v in m.named_parameters()}, g64)
    worst = max(err, key=err.get)
    print(f"worst gradient {worst} rel {err[worst]:.3e} (gate {tol:.3e})")
    for k, ref in v64.items():
        assert abs(got[k] - ref) <= tol_term[k] * abs(ref), k
    assert set(err) == {k for k, _ in m.named_parameters()} and err[worst] <= tol, (worst, err[worst])
    ts.close()
