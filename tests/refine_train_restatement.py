"""A torch restatement of the refiner trunk's TRAINING forward (reference model/segment_refine_model.py:175-217 under train(), the
hand->object distance supplied) that accepts injected dropout keep-masks, for the tests of libtamf_refinetrain.so.  oracle/
mdm_oracle.refine_forward is the same function without dropout; test_refinetrain_cpu.py holds the two together at p = 0.

masks: {site: bool (B, rows, cols)} with the sites of include/tamf_refinetrain.h (S = T + 3, d = latent_dim):
    0 x + PE (S, d); 1 + 4l attention probabilities (H * S head-major, S); 2 + 4l out-projection output (S, d); 3 + 4l GELU output
    (S, ff); 4 + 4l linear2 output (S, d).  A missing site keeps everything.  Kept values are scaled by 1 / (1 - p).
obj_num: per-clip object counts (the mean over a clip's own objects) or None (the mean over all padded rows, the reference's forward).
"""
import hashlib
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import mdm_oracle as mo  # noqa: E402


def _lin(sd, name, x):
    return x @ sd[f"{name}.weight"].to(x.dtype).t() + sd[f"{name}.bias"].to(x.dtype)


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w.to(x.dtype) + b.to(x.dtype)


def _object_mean(x, obj_num):
    """(B, nobj, ...) -> (B, ...): over all rows, or over each clip's first obj_num[b]"""
    if obj_num is None:
        return x.mean(dim=1)
    return torch.stack([x[b, : int(n)].mean(dim=0) for b, n in enumerate(obj_num)], dim=0)


def refine_train_forward(sd, arch, sample_pose_repr, h2o_dist, cond, dtype=torch.float64, masks=None, p=0.0, obj_num=None):
    """-> refine_pose_repr (B, T, input_dim).  sd: state dict (tensors may require grad); cond: "hand_side", "shape", "obj_embedding",
    "obj_traj" as oracle.mdm_oracle.refine_forward takes them."""
    masks = masks or {}
    keep_scale = 1.0 / (1.0 - p)

    def drop(x, site, shape=None):
        if site not in masks:
            return x
        m = masks[site].to(device=x.device, dtype=x.dtype)
        return x * (m.reshape(shape) if shape is not None else m) * keep_scale

    dt = dtype
    d, H = arch.latent_dim, arch.num_heads
    hd = d // H
    x_in = sample_pose_repr.to(dt)
    B, T, _ = x_in.shape
    S = T + 3
    pe = sd["sequence_pos_encoder.pe"][:, 0, :].to(dt)
    rows = [sd["hand_side_process.rh_embed" if hs in ("rh", 0) else "hand_side_process.lh_embed"] for hs in cond["hand_side"]]
    e_side = torch.stack(rows, dim=0).to(dt)
    e_shp = _lin(sd, "hand_shape_process.shape_embed", cond["shape"].to(dt).mean(dim=1))
    e_obj = _lin(sd, "obj_embed_process.embedding", _object_mean(cond["obj_embedding"].to(dt), obj_num))
    prefix = torch.nan_to_num(torch.stack([e_side, e_shp, e_obj], dim=1))
    hand = _lin(sd, "input_process.poseEmbedding", x_in)
    obj = _lin(sd, "obj_input_process.poseEmbedding", _object_mean(cond["obj_traj"].to(dt), obj_num))
    dist = _lin(sd, "h2o_dist_input_process.poseEmbedding", h2o_dist.to(dt))
    z = _lin(sd, "input_merge.0", torch.cat([hand, obj, dist], dim=-1))
    h = torch.nan_to_num(_lin(sd, "input_merge.2", z * torch.sigmoid(z)))
    seq = drop(torch.cat([prefix, h], dim=1) + pe[:S].unsqueeze(0), 0)
    for l in range(arch.num_layers):
        q = f"seqTransEncoder.layers.{l}"
        qkv = seq @ sd[f"{q}.self_attn.in_proj_weight"].to(dt).t() + sd[f"{q}.self_attn.in_proj_bias"].to(dt)
        qq, kk, vv = (t.view(B, S, H, hd).transpose(1, 2) for t in qkv.split(d, dim=-1))
        att = drop(torch.softmax((qq @ kk.transpose(-1, -2)) / math.sqrt(hd), dim=-1), 1 + 4 * l, (B, H, S, S))
        a = _lin(sd, f"{q}.self_attn.out_proj", (att @ vv).transpose(1, 2).reshape(B, S, d))
        seq = _ln(seq + drop(a, 2 + 4 * l), sd[f"{q}.norm1.weight"], sd[f"{q}.norm1.bias"])
        u = _lin(sd, f"{q}.linear1", seq)
        g = drop(0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0))), 3 + 4 * l)
        seq = _ln(seq + drop(_lin(sd, f"{q}.linear2", g), 4 + 4 * l), sd[f"{q}.norm2.weight"], sd[f"{q}.norm2.bias"])
    return torch.nan_to_num(x_in + _lin(sd, "output_process.poseFinal", seq[:, 3:, :]))


# ---- seeded cases, float64 autograd, fixtures ----
BUFFERS = ("hand_side_process.rh_embed", "hand_side_process.lh_embed", "sequence_pos_encoder.pe")
ARCH_NAMES = ("input_dim", "obj_input_dim", "hand_shape_dim", "obj_embed_dim", "latent_dim", "ff_size", "num_layers", "num_heads", "h2o_dim")
ARCH_TINY = mo.Arch(latent_dim=128, ff_size=256, num_layers=2, num_heads=2, obj_embed_dim=32, kind="R")
ARCH_L1 = mo.Arch(latent_dim=64, ff_size=16, num_layers=1, num_heads=1, obj_embed_dim=32, kind="R")
ARCH_DEEP = mo.Arch(latent_dim=64, ff_size=64, num_layers=8, num_heads=1, obj_embed_dim=32, kind="R")
PE_ROWS = 256


def arch_dict(arch):
    return {k: int(getattr(arch, k)) for k in ARCH_NAMES}


def arch_of(values):
    return mo.Arch(kind="R", **dict(zip(ARCH_NAMES, (int(v) for v in values))))


def seeded_state_dict(arch, seed):
    """{key: float32 array} of the R state dict: PyTorch-default magnitudes, LayerNorm gains 1 + U(-0.1, 0.1), biases U(-0.05, 0.05),
    hand-side rows as the module's, the PE table as the module's"""
    rng = np.random.default_rng(seed)
    spec = mo.state_dict_spec(arch)
    sd = {}
    for name, shape in spec.items():
        if name.endswith(".pe"):
            sd[name] = mo.positional_table(arch.latent_dim).unsqueeze(1).numpy().copy()
        elif name.endswith("rh_embed"):
            sd[name] = np.zeros(shape, np.float32)
        elif name.endswith("lh_embed"):
            sd[name] = np.eye(1, shape[0], dtype=np.float32)[0]
        elif ".norm" in name:
            sd[name] = ((1.0 if name.endswith("weight") else 0.0) + rng.uniform(-1, 1, shape) * (0.1 if name.endswith("weight") else 0.05)).astype(np.float32)
        else:
            fan_in = shape[1] if len(shape) == 2 else spec[name.replace("in_proj_bias", "in_proj_weight").replace(".bias", ".weight")][1]
            sd[name] = (rng.uniform(-1, 1, shape) / math.sqrt(fan_in)).astype(np.float32)
    return sd


def seeded_inputs(arch, B, T, nobj, seed, ragged=False):
    """sample_pose_repr, h2o_dist (non-negative, centimetres), shape (constant over a clip's frames), obj_embedding, obj_traj, hand
    sides rh / lh / rh ..., and obj_num (ragged: 1 + b % nobj) or None"""
    rng = np.random.default_rng(seed)
    inp = {"sample_pose_repr": rng.normal(0, 0.5, (B, T, arch.input_dim)).astype(np.float32),
           "h2o_dist": np.abs(rng.normal(0, 0.05, (B, T, arch.h2o_dim))).astype(np.float32),
           "shape": np.repeat(rng.normal(0, 1, (B, 1, arch.hand_shape_dim)), T, axis=1).astype(np.float32),
           "obj_embedding": rng.normal(0, 1, (B, nobj, arch.obj_embed_dim)).astype(np.float32),
           "obj_traj": rng.normal(0, 0.5, (B, nobj, T, arch.obj_input_dim)).astype(np.float32),
           "hand_side": ["lh" if b % 2 else "rh" for b in range(B)]}
    return inp, ([1 + (b + 1) % nobj for b in range(B)] if ragged else None)


def cond_of(inp, dtype=torch.float64, rows=None):
    sl = slice(None) if rows is None else rows
    c = {k: torch.from_numpy(np.ascontiguousarray(inp[k][sl])).to(dtype) for k in ("shape", "obj_embedding", "obj_traj")}
    c["hand_side"] = list(np.asarray(inp["hand_side"])[sl]) if rows is not None else list(inp["hand_side"])
    return c


def leaf_state_dict(sd_np, dtype=torch.float64):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).clone().requires_grad_(k not in BUFFERS) for k, v in sd_np.items()}


def loss_and_grads(sd_np, arch, inp, G, obj_num=None, masks=None, p=0.0, dtype=torch.float64, forward=None):
    """loss = sum(G * refine_pose_repr) -> (out float64 array, loss float, {key: gradient float64}); `forward` defaults to the
    restatement, oracle_forward runs oracle.mdm_oracle.refine_forward (no dropout, clip by clip when obj_num is given)"""
    sd = leaf_state_dict(sd_np, dtype)
    x, h = torch.from_numpy(inp["sample_pose_repr"]).to(dtype), torch.from_numpy(inp["h2o_dist"]).to(dtype)
    if forward is None:
        out = refine_train_forward(sd, arch, x, h, cond_of(inp, dtype), dtype, masks, p, obj_num)
    else:
        out = forward(sd, arch, x, h, inp, dtype, obj_num)
    loss = (torch.from_numpy(np.asarray(G)).to(dtype) * out).sum()
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy() for k, v in sd.items() if k not in BUFFERS}
    return out.detach().double().numpy(), float(loss.detach()), grads


def oracle_forward(sd, arch, x, h, inp, dtype, obj_num):
    if obj_num is None:
        return mo.refine_forward(sd, arch, x, h, cond_of(inp, dtype), dtype)
    outs = []
    for b, n in enumerate(obj_num):
        c = cond_of(inp, dtype, rows=slice(b, b + 1))
        c["obj_embedding"], c["obj_traj"] = c["obj_embedding"][:, : int(n)], c["obj_traj"][:, : int(n)]
        outs.append(mo.refine_forward(sd, arch, x[b : b + 1], h[b : b + 1], c, dtype))
    return torch.cat(outs, dim=0)


def rel_err(got, ref):
    """|got - ref|_inf / |ref|_inf over the finite entries of ref; NaN entries have to be NaN in both (inf when they are not)"""
    r, g = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    nan = np.isnan(r)
    if (np.isnan(g) != nan).any():
        return float("inf")
    if nan.all():
        return 0.0
    den = np.nanmax(np.abs(r))
    return float(np.nanmax(np.abs(g - r)) / (den if den > 0 else 1.0))


def grad_rel_err(got, ref):
    return {k: rel_err(got[k], r) for k, r in ref.items()}


def site_shapes(arch, T):
    """{site: (rows, cols)} of every dropout site of a clip of T frames"""
    S, d, ff, H = T + 3, arch.latent_dim, arch.ff_size, arch.num_heads
    out = {0: (S, d)}
    for l in range(arch.num_layers):
        out.update({1 + 4 * l: (H * S, S), 2 + 4 * l: (S, d), 3 + 4 * l: (S, ff), 4 + 4 * l: (S, d)})
    return out


def sd_digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()


def load_case(path):
    """a tests/golden/refinetrain_*.npz fixture -> {"arch", "sd", "inputs", "obj_num", "G" (trunk fixtures), "out", "loss", "grads"
    (every gstride-th element of the flattened float64 gradient), "gstride", "gmax" (the whole tensor's max-norm), "tol_rel",
    "tol_rel_out", "tol_rel_loss", "z" (the file)}; the weights are regenerated from `sd_seed` and checked against `sd_sha256`"""
    z = np.load(path, allow_pickle=False)
    arch = arch_of(z["arch"])
    sd = seeded_state_dict(arch, int(z["sd_seed"]))
    assert sd_digest({k: v for k, v in sd.items() if not k.endswith(".pe")}) == str(z["sd_sha256"]), "the regenerated weights differ from the fixture's"
    head = z["pe_head"]
    assert np.abs(sd["sequence_pos_encoder.pe"][: head.shape[0], 0] - head).max() <= 1e-5
    sd["sequence_pos_encoder.pe"][: head.shape[0], 0] = head
    inputs = {k[3:]: z[k] for k in z.files if k.startswith("in/") and k != "in/obj_num"}
    inputs["hand_side"] = [str(s) for s in inputs["hand_side"]]
    return {"arch": arch, "sd": sd, "inputs": inputs, "obj_num": [int(v) for v in z["in/obj_num"]] if "in/obj_num" in z.files else None,
            "G": z["G"] if "G" in z.files else None, "out": z["out"], "loss": float(z["loss"]),
            "grads": {k[5:]: z[k] for k in z.files if k.startswith("grad/")}, "gstride": {k[8:]: int(z[k]) for k in z.files if k.startswith("gstride/")},
            "gmax": {k[5:]: float(z[k]) for k in z.files if k.startswith("gmax/")}, "tol_rel": float(z["tol_rel"]),
            "tol_rel_out": float(z["tol_rel_out"]), "tol_rel_loss": float(z["tol_rel_loss"]), "z": z}


def fixture_grad_err(got, case):
    """{key: max over the fixture's samples of |got - ref| / the whole reference tensor's max-norm}; every trainable key has to be there"""
    assert set(got) == set(case["grads"]) and not set(got) & set(BUFFERS)
    out = {}
    for k, ref in case["grads"].items():
        g = np.asarray(got[k], np.float64).reshape(-1)[:: case["gstride"][k]]
        assert g.shape == ref.shape
        out[k] = float(np.abs(g - ref).max() / case["gmax"][k]) if case["gmax"][k] > 0 else float(np.abs(g - ref).max())
    return out
