"""A torch restatement of the denoiser G's TRAINING forward (reference model/interaction_segment_mdm.py:134-174 under train(), the CLIP
text features supplied) that accepts injected dropout keep-masks, for the tests of libtamf_mdmtrain.so.  oracle/mdm_oracle.
denoiser_forward is the same function without dropout; test_mdmtrain_cpu.py holds the two together at p = 0.

masks: {site: bool (B, rows, cols)} with the sites of include/tamf_mdmtrain.h (S = T + 5, d = latent_dim):
    0 x + PE (S, d); 1 + 4l attention probabilities (H * S head-major, S); 2 + 4l out-projection output (S, d); 3 + 4l GELU output
    (S, ff); 4 + 4l linear2 output (S, d).  A missing site keeps everything.  Kept values are scaled by 1 / (1 - p).
obj_num: per-clip object counts (the mean over a clip's own objects) or None (the mean over all padded rows, the reference's forward).

What does not depend on the model (the linear map, LayerNorm, the object mean, the error measures, the fixture's gradient samples) is
refine_train_restatement's.
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_train_restatement as R  # noqa: E402

mo = R.mo
rel_err, grad_rel_err, sd_digest, fixture_grad_err = R.rel_err, R.grad_rel_err, R.sd_digest, R.fixture_grad_err
PREFIX = 5


def mdm_train_forward(sd, arch, x_t, t, cond, dtype=torch.float64, masks=None, p=0.0, obj_num=None):
    """-> model_output (B, input_dim, 1, T).  sd: state dict (tensors may require grad); x_t (B, input_dim, 1, T); t (B,) integers; cond:
    "text_embedding", "hand_side", "shape", "obj_embedding", "obj_traj" as oracle.mdm_oracle.denoiser_forward takes them."""
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
    x_in = x_t.to(dt)[:, :, 0, :].transpose(1, 2)  # (B, T, F)
    B, T, _ = x_in.shape
    S = T + PREFIX
    pe = sd["sequence_pos_encoder.pe"][:, 0, :].to(dt)
    z = R._lin(sd, "embed_timestep.time_embed.0", pe[torch.as_tensor(t).long()])
    e_t = R._lin(sd, "embed_timestep.time_embed.2", z * torch.sigmoid(z))
    e_txt = R._lin(sd, "embed_text", cond["text_embedding"].to(dt))
    rows = [sd["hand_side_process.rh_embed" if hs in ("rh", 0) else "hand_side_process.lh_embed"] for hs in cond["hand_side"]]
    e_side = torch.stack(rows, dim=0).to(dt)
    e_shp = R._lin(sd, "hand_shape_process.shape_embed", cond["shape"].to(dt).mean(dim=1))
    e_obj = R._lin(sd, "obj_embed_process.embedding", R._object_mean(cond["obj_embedding"].to(dt), obj_num))
    prefix = torch.nan_to_num(torch.stack([e_t, e_txt, e_side, e_shp, e_obj], dim=1))
    hand = R._lin(sd, "input_process.poseEmbedding", x_in)
    obj = R._lin(sd, "obj_input_process.poseEmbedding", R._object_mean(cond["obj_traj"].to(dt), obj_num))
    z = R._lin(sd, "input_merge.0", torch.cat([hand, obj], dim=-1))
    h = torch.nan_to_num(R._lin(sd, "input_merge.2", z * torch.sigmoid(z)))
    seq = drop(torch.cat([prefix, h], dim=1) + pe[:S].unsqueeze(0), 0)
    for l in range(arch.num_layers):
        q = f"seqTransEncoder.layers.{l}"
        qkv = seq @ sd[f"{q}.self_attn.in_proj_weight"].to(dt).t() + sd[f"{q}.self_attn.in_proj_bias"].to(dt)
        qq, kk, vv = (u.view(B, S, H, hd).transpose(1, 2) for u in qkv.split(d, dim=-1))
        att = drop(torch.softmax((qq @ kk.transpose(-1, -2)) / math.sqrt(hd), dim=-1), 1 + 4 * l, (B, H, S, S))
        a = R._lin(sd, f"{q}.self_attn.out_proj", (att @ vv).transpose(1, 2).reshape(B, S, d))
        seq = R._ln(seq + drop(a, 2 + 4 * l), sd[f"{q}.norm1.weight"], sd[f"{q}.norm1.bias"])
        u = R._lin(sd, f"{q}.linear1", seq)
        g = drop(0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0))), 3 + 4 * l)
        seq = R._ln(seq + drop(R._lin(sd, f"{q}.linear2", g), 4 + 4 * l), sd[f"{q}.norm2.weight"], sd[f"{q}.norm2.bias"])
    out = torch.nan_to_num(R._lin(sd, "output_process.poseFinal", seq[:, PREFIX:, :]))
    return out.transpose(1, 2).unsqueeze(2)


# ---- seeded cases, float64 autograd, fixtures ----
BUFFERS = ("hand_side_process.rh_embed", "hand_side_process.lh_embed", "sequence_pos_encoder.pe", "embed_timestep.sequence_pos_encoder.pe")
ARCH_NAMES = ("input_dim", "obj_input_dim", "hand_shape_dim", "obj_embed_dim", "latent_dim", "ff_size", "num_layers", "num_heads", "clip_dim")
ARCH_L1_64 = mo.Arch(latent_dim=64, ff_size=16, num_layers=1, num_heads=1, obj_embed_dim=32, clip_dim=16)
ARCH_L1_128 = mo.Arch(latent_dim=128, ff_size=16, num_layers=1, num_heads=1, obj_embed_dim=32, clip_dim=16)
ARCH_TINY_64 = mo.Arch(latent_dim=128, ff_size=256, num_layers=2, num_heads=2, obj_embed_dim=32, clip_dim=16)
ARCH_TINY_128 = mo.Arch(latent_dim=256, ff_size=256, num_layers=2, num_heads=2, obj_embed_dim=32, clip_dim=16)
PE_ROWS = 256
FLOAT_INPUTS = ("x_t", "text_embedding", "shape", "obj_embedding", "obj_traj")


def arch_dict(arch):
    return {k: int(getattr(arch, k)) for k in ARCH_NAMES}


def arch_of(values):
    return mo.Arch(kind="G", **dict(zip(ARCH_NAMES, (int(v) for v in values))))


def seeded_state_dict(arch, seed):
    """{key: float32 array} of the G state dict, by refine_train_restatement.seeded_state_dict's recipe (both PE keys hold the table)"""
    assert arch.kind == "G"
    return R.seeded_state_dict(arch, seed)


def seeded_inputs(arch, B, T, nobj, seed, ragged=False):
    """x_t (B, input_dim, 1, T), t (B,) in [0, 1000), text_embedding, shape (constant over a clip's frames), obj_embedding, obj_traj,
    hand sides rh / lh / rh ..., and obj_num (ragged) or None"""
    rng = np.random.default_rng(seed)
    inp = {"x_t": rng.normal(0, 0.7, (B, arch.input_dim, 1, T)).astype(np.float32),
           "t": rng.integers(0, 1000, (B,)).astype(np.int64),
           "text_embedding": rng.normal(0, 1, (B, arch.clip_dim)).astype(np.float32),
           "shape": np.repeat(rng.normal(0, 1, (B, 1, arch.hand_shape_dim)), T, axis=1).astype(np.float32),
           "obj_embedding": rng.normal(0, 1, (B, nobj, arch.obj_embed_dim)).astype(np.float32),
           "obj_traj": rng.normal(0, 0.5, (B, nobj, T, arch.obj_input_dim)).astype(np.float32),
           "hand_side": ["lh" if b % 2 else "rh" for b in range(B)]}
    return inp, ([1 + (b + 1) % nobj for b in range(B)] if ragged else None)


def cond_of(inp, dtype=torch.float64, rows=None):
    sl = slice(None) if rows is None else rows
    c = {k: torch.from_numpy(np.ascontiguousarray(inp[k][sl])).to(dtype) for k in ("text_embedding", "shape", "obj_embedding", "obj_traj")}
    c["hand_side"] = list(np.asarray(inp["hand_side"])[sl]) if rows is not None else list(inp["hand_side"])
    return c


def leaf_state_dict(sd_np, dtype=torch.float64):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).clone().requires_grad_(k not in BUFFERS) for k, v in sd_np.items()}


def loss_and_grads(sd_np, arch, inp, G, obj_num=None, masks=None, p=0.0, dtype=torch.float64, forward=None):
    """loss = sum(G * model_output), G (B, input_dim, 1, T) -> (out float64 array, loss float, {key: gradient float64}); `forward`
    defaults to the restatement, oracle_forward runs oracle.mdm_oracle.denoiser_forward (no dropout, clip by clip when obj_num is given)"""
    sd = leaf_state_dict(sd_np, dtype)
    x, t = torch.from_numpy(inp["x_t"]).to(dtype), torch.from_numpy(np.asarray(inp["t"]))
    if forward is None:
        out = mdm_train_forward(sd, arch, x, t, cond_of(inp, dtype), dtype, masks, p, obj_num)
    else:
        out = forward(sd, arch, x, t, inp, dtype, obj_num)
    loss = (torch.from_numpy(np.asarray(G)).to(dtype) * out).sum()
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy() for k, v in sd.items() if k not in BUFFERS}
    return out.detach().double().numpy(), float(loss.detach()), grads


def oracle_forward(sd, arch, x, t, inp, dtype, obj_num):
    if obj_num is None:
        return mo.denoiser_forward(sd, arch, x, t, cond_of(inp, dtype), dtype)
    outs = []
    for b, n in enumerate(obj_num):
        c = cond_of(inp, dtype, rows=slice(b, b + 1))
        c["obj_embedding"], c["obj_traj"] = c["obj_embedding"][:, : int(n)], c["obj_traj"][:, : int(n)]
        outs.append(mo.denoiser_forward(sd, arch, x[b : b + 1], t[b : b + 1], c, dtype))
    return torch.cat(outs, dim=0)


def site_shapes(arch, T):
    """{site: (rows, cols)} of every dropout site of a clip of T frames"""
    S, d, ff, H = T + PREFIX, arch.latent_dim, arch.ff_size, arch.num_heads
    out = {0: (S, d)}
    for l in range(arch.num_layers):
        out.update({1 + 4 * l: (H * S, S), 2 + 4 * l: (S, d), 3 + 4 * l: (S, ff), 4 + 4 * l: (S, d)})
    return out


def load_case(path):
    """a tests/golden/mdmtrain_*.npz fixture -> {"arch", "sd", "inputs", "obj_num", "G" (trunk fixtures), "out", "loss", "grads" (every
    gstride-th element of the flattened float64 gradient), "gstride", "gmax" (the whole tensor's max-norm), "tol_rel", "tol_rel_out",
    "tol_rel_loss" (where the file has them: mdmtrain_sgd.npz holds a loss curve instead), "z" (the file)}; the weights are regenerated from `sd_seed` and checked against `sd_sha256`; the PE rows the
    fixture's run read (the first PE_ROWS and the rows pe[t]) are the stored ones"""
    z = np.load(path, allow_pickle=False)
    arch = arch_of(z["arch"])
    sd = seeded_state_dict(arch, int(z["sd_seed"]))
    assert sd_digest({k: v for k, v in sd.items() if not k.endswith(".pe")}) == str(z["sd_sha256"]), "the regenerated weights differ from the fixture's"
    head, pe_t, t_rows = z["pe_head"], z["pe_t"], z["pe_t_rows"]
    pe = sd["sequence_pos_encoder.pe"]
    # (a sanity check of the regenerated table before the stored rows replace it.  Row r is sin / cos of r * w in float32 with w <= 1
    # from a float32 exp: two libms' w differ by up to 2 ulp, 2.4e-7 relative, which moves the phase of row r by up to 2.4e-7 r)
    assert np.abs(pe[: head.shape[0], 0] - head).max() <= 1e-5 + 2.4e-7 * head.shape[0]
    assert (np.abs(pe[t_rows, 0] - pe_t).max(axis=1) <= 1e-5 + 2.4e-7 * t_rows).all()
    pe[: head.shape[0], 0] = head
    pe[t_rows, 0] = pe_t
    sd["embed_timestep.sequence_pos_encoder.pe"] = pe
    inputs = {k[3:]: z[k] for k in z.files if k.startswith("in/") and k != "in/obj_num"}
    inputs["hand_side"] = [str(s) for s in inputs["hand_side"]]
    return {"arch": arch, "sd": sd, "inputs": inputs, "obj_num": [int(v) for v in z["in/obj_num"]] if "in/obj_num" in z.files else None,
            "G": z["G"] if "G" in z.files else None, "out": z["out"] if "out" in z.files else None,
            "grads": {k[5:]: z[k] for k in z.files if k.startswith("grad/")}, "gstride": {k[8:]: int(z[k]) for k in z.files if k.startswith("gstride/")},
            "gmax": {k[5:]: float(z[k]) for k in z.files if k.startswith("gmax/")}, "z": z,
            **{k: float(z[k]) for k in ("loss", "tol_rel", "tol_rel_out", "tol_rel_loss") if k in z.files}}  # (mdmtrain_sgd.npz holds a curve instead)


def module_state_dict(sd_np):
    """{key: float32 tensor} as InterationSegmentMDM.load_state_dict takes it"""
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd_np.items()}
