"""Capture the refiner training fixtures (tests/golden/refinetrain_*.npz) from the reference.

Run where a checkout of the reference is available (CPU only):  python tools/capture_refinetrain_golden.py REFERENCE_ROOT

The reference's own SegmentRefineModel (model/segment_refine_model.py) is imported as it is (the stand-ins of
tools/capture_contact_golden.py for manotorch, pytorch3d and chamfer_distance, those of tools/capture_encoder_golden.py for what it
imports but does not use) and run in train() mode with dropout 0.0, in float64 and
in float32.

Trunk fixtures (refinetrain_tiny / _l1_ff16 / _deep .npz): the module's batch_recover_mano_from_pose_repr is replaced by a no-op and
its multi_object_h2o_dist by a function that returns a seeded tensor, so the files pin the trunk alone; the loss is sum(G * refine_pose_repr)
with a seeded G.  With a ragged obj_num the module is run one clip at a time on the clip's own objects.

refinetrain_e2e.npz: nothing replaced.  Tiny architecture, B 2 (rh, lh), T 5, masks 5 / 3, 2 / 1 objects of P = 96 points (the recipe
of capture_contact_golden.py around the ground-truth hand), synthetic 778-vertex MANO arrays; the loss is the reference's
SegmentRefineModelLoss with config/loss_param_refine.yml's coefficients (1.0 / 1.0 / 0.1).  Conditions, asserted on what the
reference's point2point_signed saw (another seed is tried when one fails): the float32 and float64 runs choose identical nearest
object points for every hand vertex, and the relative gap between nearest and second-nearest squared distance is >= 1e-5.

Each file holds the float32 inputs, the seed the weights are regenerated from (and their SHA-256), the reference's float64 output, loss
and parameter gradients, per quantity e32_* = the deviation of the reference's float32 run from its float64 run (max-norm relative per
tensor) and the gates tol_rel* = 4 * e32 (another valid fp32 summation order may sit a small multiple of that distance away).  A
gradient of more than GRAD_KEEP elements is stored as every stride-th element of the flattened tensor (a prime stride, so that the
samples walk through every position of a kernel's tile) with the max-norm of the whole tensor.  Data only: no program text of the
reference is stored, and no MANO array."""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oakink2-tamf_amd"))
import capture_contact_golden as CC  # noqa: E402
import capture_recloss_golden as CR  # noqa: E402
import contact_restatement as CS  # noqa: E402
import mano_fixture as MF  # noqa: E402
import refine_train_restatement as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
GRAD_KEEP = 2048
PRIMES = (1, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101)
COEF = dict(coef_rec_joint_loss=1.0, coef_rec_vert_loss=1.0, coef_dist_h_loss=0.1)  # the reference's config/loss_param_refine.yml
_records = []


def build(Model, arch, sd, dtype):
    assert arch.h2o_dim == 778
    model = Model("unused", input_dim=arch.input_dim, obj_input_dim=arch.obj_input_dim, hand_shape_dim=arch.hand_shape_dim,
                  obj_embed_dim=arch.obj_embed_dim, latent_dim=arch.latent_dim, ff_size=arch.ff_size, num_layers=arch.num_layers,
                  num_heads=arch.num_heads, dropout=0.0).train()
    own = {k: v for k, v in model.state_dict().items() if k.startswith("mano_layer_")}
    missing, unexpected = model.load_state_dict({**own, **{k: torch.from_numpy(v) for k, v in sd.items()}}, strict=True)
    assert not missing and not unexpected
    return model.to(dtype)


def batch_of(inp, dtype, rows=None, nobj=None):
    sl = slice(None) if rows is None else rows
    b = {k: torch.from_numpy(inp[k][sl]).to(dtype) for k in ("sample_pose_repr", "shape", "obj_embedding", "obj_traj")}
    if nobj is not None:
        b["obj_embedding"], b["obj_traj"] = b["obj_embedding"][:, :nobj], b["obj_traj"][:, :nobj]
    b["hand_side"] = list(inp["hand_side"][sl]) if rows is not None else list(inp["hand_side"])
    b["pose_repr"] = b["sample_pose_repr"]
    b["obj_list"], b["obj_verts"] = [[]] * len(b["hand_side"]), [[]] * len(b["hand_side"])
    return b


def trunk_run(Model, arch, sd, inp, obj_num, G, dtype):
    """-> out (B, T, F) float64, loss, {key: gradient float64}"""
    model = build(Model, arch, sd, dtype)
    model.batch_recover_mano_from_pose_repr = lambda *a: (None, None, None)
    outs = []
    for rows, nobj in ([(None, None)] if obj_num is None else [(slice(b, b + 1), int(n)) for b, n in enumerate(obj_num)]):
        h2o = torch.from_numpy(inp["h2o_dist"][rows if rows is not None else slice(None)]).to(dtype)
        calls = [0]

        def dist(*a, h2o=h2o, calls=calls):  # the first call is the sample's feature; the later ones feed the loss, unused here
            calls[0] += 1
            return h2o if calls[0] == 1 else torch.zeros_like(h2o)

        model.multi_object_h2o_dist = dist
        outs.append(model(batch_of(inp, dtype, rows, nobj))["refine_pose_repr"])
    out = torch.cat(outs, dim=0)
    loss = (torch.from_numpy(G).to(dtype) * out).sum()
    loss.backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).double().numpy() for k, p in model.named_parameters()}
    return out.detach().double().numpy(), float(loss.detach()), grads


def compact(grads):
    """{grad/<key>: samples float64, gmax/<key>: the whole tensor's max-norm, gstride/<key>}"""
    out = {}
    for k, g in grads.items():
        stride = next(p for p in PRIMES if g.size <= GRAD_KEEP * p)
        out[f"grad/{k}"] = g.reshape(-1)[::stride].copy()
        out[f"gmax/{k}"] = np.float64(np.abs(g).max())
        out[f"gstride/{k}"] = np.int32(stride)
    return out


def rel(a32, a64):
    return float(np.abs(a32 - a64).max() / np.abs(a64).max())


def common(arch, sd, sd_seed, inp, obj_num):
    data = {"arch": np.array([getattr(arch, k) for k in R.ARCH_NAMES], np.int32), "pe_head": sd["sequence_pos_encoder.pe"][: R.PE_ROWS, 0],
            "sd_seed": np.int64(sd_seed), "sd_sha256": np.array(R.sd_digest({k: v for k, v in sd.items() if not k.endswith(".pe")}))}
    for k in ("sample_pose_repr", "h2o_dist", "shape", "obj_embedding", "obj_traj"):
        if k in inp:
            data[f"in/{k}"] = inp[k]
    data["in/hand_side"] = np.array(inp["hand_side"])
    if obj_num is not None:
        data["in/obj_num"] = np.asarray(obj_num, np.int32)
    return data


def gates(g32, g64, o32, o64, l32, l64):
    e = {k: rel(g32[k], g64[k]) for k in g64 if np.abs(g64[k]).max() > 0}
    e_out, e_loss = rel(o32, o64), max(abs(l32 - l64) / abs(l64), 2.0 ** -24)
    return {"e32_grad": np.float64(max(e.values())), "e32_out": np.float64(e_out), "e32_loss": np.float64(e_loss),
            "tol_rel": np.float64(4 * max(e.values())), "tol_rel_out": np.float64(4 * e_out), "tol_rel_loss": np.float64(4 * e_loss),
            **{f"e32/{k}": np.float64(v) for k, v in e.items()}}


def save(name, data):
    path = os.path.join(GOLDEN, name)
    np.savez_compressed(path, **data)
    print(f"{name}: loss {float(data['loss']):.6f} e32_grad {float(data['e32_grad']):.3e} tol_rel {float(data['tol_rel']):.3e} tol_rel_out "
          f"{float(data['tol_rel_out']):.3e} tol_rel_loss {float(data['tol_rel_loss']):.3e} {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1000000


def capture_trunk(Model, name, arch, sd_seed, in_seed, B, T, nobj, ragged, mask_len=None):
    sd = R.seeded_state_dict(arch, sd_seed)
    inp, obj_num = R.seeded_inputs(arch, B, T, nobj, in_seed, ragged)
    G = np.random.default_rng(in_seed + 1).normal(size=(B, T, arch.input_dim)).astype(np.float32)
    if mask_len is not None:  # ragged masks: the frames past a clip's length carry no loss
        G *= (np.arange(T)[None, :] < np.asarray(mask_len)[:, None])[:, :, None]
    o64, l64, g64 = trunk_run(Model, arch, sd, inp, obj_num, G, torch.float64)
    o32, l32, g32 = trunk_run(Model, arch, sd, inp, obj_num, G, torch.float32)
    assert not set(g64) & set(R.BUFFERS)
    save(name, {**common(arch, sd, sd_seed, inp, obj_num), "G": G, "out": o64, "loss": np.float64(l64), **compact(g64), **gates(g32, g64, o32, o64, l32, l64)})


# ---- the end-to-end fixture ----
E2E = dict(B=2, T=5, MASK_LEN=(5, 3), SIDES=("rh", "lh"), OBJ_NUM=(2, 1))


def record_calls(module):
    inner = module.point2point_signed

    def point2point_signed(x, y, x_normals=None, y_normals=None):
        out = inner(x, y, x_normals, y_normals)
        _records.append(dict(x=x.detach().double(), y=y.detach().double(), idx=CS.sq_dists(x.detach(), y.detach()).argmin(dim=2)))
        return out

    module.point2point_signed = point2point_signed


def e2e_run(Model, Loss, cfg, arch, sd, arrays, objects, dtype):
    CR._dtype[0] = dtype
    _records.clear()
    model = build(Model, arch, sd, dtype)
    crit = Loss(cfg).to(dtype)
    sample, gt, shape, mask, oemb = (torch.from_numpy(a).to(dtype) for a in arrays)
    traj, pts = objects
    n = E2E["OBJ_NUM"]
    outs = []
    for b in range(E2E["B"]):  # one clip at a time on the clip's own objects
        batch = {"sample_pose_repr": sample[b:b + 1], "pose_repr": gt[b:b + 1], "shape": shape[b:b + 1], "hand_side": [E2E["SIDES"][b]],
                 "obj_embedding": oemb[b:b + 1, :n[b]], "obj_traj": torch.from_numpy(traj[b:b + 1, :n[b]]).to(dtype), "obj_list": [list(range(n[b]))],
                 "obj_verts": [pts[b, :n[b]]]}
        outs.append(model(batch))
    output = {k: torch.cat([o[k] for o in outs], dim=0) for k in outs[0]}
    loss, d = crit(output, {"mask": mask})
    loss.backward()
    res = {k: float(d[k]) for k in ("loss", "rec_joint", "rec_vert", "dist_h")}
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).double().numpy() for k, p in model.named_parameters()}
    return res, output["refine_pose_repr"].detach().double().numpy(), grads, list(_records)


def e2e_conditions(rec64, rec32):
    same, gap = len(rec64) == len(rec32), np.inf
    for r64, r32 in zip(rec64, rec32):
        same &= bool(torch.equal(r64["idx"], r32["idx"]))
        two = torch.topk(CS.sq_dists(r64["x"], r64["y"]), 2, dim=-1, largest=False).values
        gap = min(gap, float(((two[..., 1] - two[..., 0]) / two[..., 1]).min()))
    return bool(same and gap >= 1e-5), dict(same=bool(same), gap=gap)


def capture_e2e(Model, Loss, mod, name, arch, sd_seed):
    for k, v in E2E.items():
        setattr(CC, k, v)
    record_calls(mod)
    sd = R.seeded_state_dict(arch, sd_seed)
    vw = CR.v_weights_of()
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "vpe.npy"), CR.unique_edges(MF.synthetic_arrays(CC.V, 0)["faces"]))
        np.save(os.path.join(tmp, "w.npy"), vw)
        cfg = dict(COEF, vpe_path=os.path.join(tmp, "vpe.npy"), c_weight_path=os.path.join(tmp, "w.npy"))
        for seed in range(64):
            pred, gt, shape, mask = CC.segment_inputs(seed)
            sample = np.ascontiguousarray(pred[:, :, 0, :].transpose(0, 2, 1))
            obj = CC.object_inputs(seed, gt, shape)
            oemb = np.random.default_rng(6100 + seed).normal(size=(E2E["B"], CC.NOBJ, arch.obj_embed_dim)).astype(np.float32)
            oemb[1, 1:] = 0.0  # (padded rows)
            arrays = (sample, gt, shape, mask, oemb)
            r64, o64, g64, rec64 = e2e_run(Model, Loss, cfg, arch, sd, arrays, obj, torch.float64)
            r32, o32, g32, rec32 = e2e_run(Model, Loss, cfg, arch, sd, arrays, obj, torch.float32)
            ok, fig = e2e_conditions(rec64, rec32)
            print(f"e2e seed {seed}: {'accepted' if ok else 'rejected'} {fig}")
            if ok:
                break
        else:
            raise SystemExit("no seed met the fixture conditions")
    inp = {"sample_pose_repr": sample, "shape": shape, "obj_embedding": oemb, "obj_traj": obj[0], "hand_side": list(E2E["SIDES"])}
    terms = {f"term/{k}": np.float64(v) for k, v in r64.items()}
    e_terms = {f"e32_term/{k}": np.float64(max(abs(r32[k] - v) / abs(v), 2.0 ** -24)) for k, v in r64.items()}
    data = {**common(arch, sd, sd_seed, inp, E2E["OBJ_NUM"]), "in/pose_repr": gt, "in/mask": mask, "in/obj_points": obj[1], "v_weights": vw,
            "seed_rh": np.int32(CR.SEEDS["right"]), "seed_lh": np.int32(CR.SEEDS["left"]), "input_seed": np.int32(seed),
            **{k: np.float64(v) for k, v in COEF.items()}, "out": o64, "loss": np.float64(r64["loss"]), **terms, **e_terms,
            "tol_rel_term": np.float64(4 * max(e_terms.values())), "cond_gap": np.float64(fig["gap"]),
            **compact(g64), **gates(g32, g64, o32, o64, r32["loss"], r64["loss"])}
    save(name, data)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    import capture_encoder_golden as ceg

    sys.path.insert(0, os.path.join(sys.argv[1], "src"))
    ceg.STUBBED = tuple(s for s in ceg.STUBBED if s != "dev_fn")  # (the reference's own dev_fn is used: rotations, transforms)
    sys.meta_path.insert(0, ceg._StubFinder())  # (what the module imports but does not use: clip, ...)
    CC.install_stand_ins()
    import oakink2_tamf.model.segment_refine_model as mod
    from oakink2_tamf.model.segment_refine_model_loss import SegmentRefineModelLoss

    Model = mod.SegmentRefineModel
    capture_trunk(Model, "refinetrain_tiny.npz", R.ARCH_TINY, 201, 202, B=3, T=14, nobj=2, ragged=True, mask_len=(14, 9, 1))
    capture_trunk(Model, "refinetrain_l1_ff16.npz", R.ARCH_L1, 211, 212, B=2, T=1, nobj=2, ragged=False)
    capture_trunk(Model, "refinetrain_deep.npz", R.ARCH_DEEP, 221, 222, B=2, T=13, nobj=2, ragged=False)
    capture_e2e(Model, SegmentRefineModelLoss, mod, "refinetrain_e2e.npz", R.ARCH_TINY, 231)


if __name__ == "__main__":
    main()
