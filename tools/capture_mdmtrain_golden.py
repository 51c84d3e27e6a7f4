"""Capture the denoiser training fixtures (tests/golden/mdmtrain_*.npz) from the reference.

Run where a checkout of the reference is available (CPU only):  python tools/capture_mdmtrain_golden.py REFERENCE_ROOT

The reference's own InterationSegmentMDM (model/interaction_segment_mdm.py) is imported as it is, with a stand-in `clip` module of
this file's own writing (a tower without parameters; nothing of CLIP is run) and its encode_text replaced by a function that returns
the fixture's text features.  It is run in train() mode with dropout 0.0, in float64 and in float32.

Trunk fixtures (mdmtrain_l1_hd64 / _l1_hd128 / _tiny_hd64 / _tiny_hd128 .npz): the loss is sum(G * model_output) with a seeded G; the
tiny ones have ragged objects (the module is run one clip at a time on the clip's own objects) and ragged masks in G.

mdmtrain_losses.npz: the reference's GaussianDiffusion.training_losses (create_gaussian_diffusion(1000, "cosine")) on the tiny hd128
model for stored x_start, t, noise and mask: its q_sample output, terms["mse"] per clip and the gradients of (terms["loss"] *
weights).mean().  mdmtrain_sgd.npz: the loss curve of 10 plain-SGD steps of that objective with stored t and noise per step.

Each trunk file holds the float32 inputs, the seed the weights are regenerated from (and their SHA-256), the PE rows the run read, the
reference's float64 output, loss and parameter gradients, per quantity e32_* = the deviation of the reference's float32 run from its
float64 run (max-norm relative per tensor) and the gates tol_rel* = 4 * e32 (another valid fp32 summation order may sit a small
multiple of that distance away).  A gradient of more than GRAD_KEEP elements is stored as every stride-th element of the flattened
tensor (a prime stride) with the max-norm of the whole tensor.  Data only: no program text of the reference is stored."""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mdm_train_restatement as M  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
GRAD_KEEP = 2048
PRIMES = (1, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127, 131)
SGD_STEPS, SGD_LR = 10, 1e-2


def install_clip_stand_in():
    """`import clip` of the reference's module: load() gives a tower without parameters, nothing else is ever called"""
    clip = types.ModuleType("clip")
    clip.model = types.ModuleType("clip.model")
    clip.model.convert_weights = lambda model: None
    clip.load = lambda version, device="cpu", jit=False: (torch.nn.Module(), None)

    def tokenize(*a, **k):
        raise RuntimeError("the stand-in clip module tokenizes nothing: encode_text is replaced by the fixture's features")

    clip.tokenize = tokenize
    sys.modules["clip"], sys.modules["clip.model"] = clip, clip.model


def build(Model, arch, sd, dtype):
    model = Model(input_dim=arch.input_dim, obj_input_dim=arch.obj_input_dim, hand_shape_dim=arch.hand_shape_dim, obj_embed_dim=arch.obj_embed_dim,
                  latent_dim=arch.latent_dim, ff_size=arch.ff_size, num_layers=arch.num_layers, num_heads=arch.num_heads, dropout=0.0,
                  clip_dim=arch.clip_dim)
    model.train()  # (the reference's override returns None)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not missing and not unexpected and model.training
    return model.to(dtype)


def batch_of(model, inp, dtype, rows=None, nobj=None):
    """the batch of the clips `rows` (all: None) on their first nobj objects; the model's encode_text returns their text features"""
    sl = slice(None) if rows is None else rows
    b = {k: torch.from_numpy(inp[k][sl]).to(dtype) for k in ("shape", "obj_embedding", "obj_traj")}
    if nobj is not None:
        b["obj_embedding"], b["obj_traj"] = b["obj_embedding"][:, :nobj], b["obj_traj"][:, :nobj]
    b["hand_side"] = list(inp["hand_side"][sl]) if rows is not None else list(inp["hand_side"])
    b["text"] = ["unused"] * len(b["hand_side"])
    text = torch.from_numpy(inp["text_embedding"][sl]).to(dtype)
    model.encode_text = lambda raw_text, text=text: text
    if "mask" in inp:
        b["mask"] = torch.from_numpy(inp["mask"][sl])
    return b


def named_grads(model):
    return {k: (p.grad if p.grad is not None else torch.zeros_like(p)).double().numpy() for k, p in model.named_parameters()}


def trunk_run(Model, arch, sd, inp, obj_num, G, dtype):
    """-> out (B, F, 1, T) float64, loss, {key: gradient float64}"""
    model = build(Model, arch, sd, dtype)
    outs = []
    for rows, nobj in ([(None, None)] if obj_num is None else [(slice(b, b + 1), int(n)) for b, n in enumerate(obj_num)]):
        sl = slice(None) if rows is None else rows
        outs.append(model(torch.from_numpy(inp["x_t"][sl]).to(dtype), torch.from_numpy(inp["t"][sl]), batch_of(model, inp, dtype, rows, nobj)))
    out = torch.cat(outs, dim=0)
    loss = (torch.from_numpy(G).to(dtype) * out).sum()
    loss.backward()
    return out.detach().double().numpy(), float(loss.detach()), named_grads(model)


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
    pe = sd["sequence_pos_encoder.pe"]
    t_rows = np.unique(np.asarray(inp["t"]).reshape(-1)).astype(np.int64)
    data = {"arch": np.array([getattr(arch, k) for k in M.ARCH_NAMES], np.int32), "pe_head": pe[: M.PE_ROWS, 0], "pe_t_rows": t_rows,
            "pe_t": pe[t_rows, 0], "sd_seed": np.int64(sd_seed),
            "sd_sha256": np.array(M.sd_digest({k: v for k, v in sd.items() if not k.endswith(".pe")}))}
    for k in M.FLOAT_INPUTS + ("t",):
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
    sd = M.seeded_state_dict(arch, sd_seed)
    inp, obj_num = M.seeded_inputs(arch, B, T, nobj, in_seed, ragged)
    G = np.random.default_rng(in_seed + 1).normal(size=(B, arch.input_dim, 1, T)).astype(np.float32)
    if mask_len is not None:  # ragged masks: the frames past a clip's length carry no loss
        G *= (np.arange(T)[None, :] < np.asarray(mask_len)[:, None])[:, None, None, :]
    o64, l64, g64 = trunk_run(Model, arch, sd, inp, obj_num, G, torch.float64)
    o32, l32, g32 = trunk_run(Model, arch, sd, inp, obj_num, G, torch.float32)
    assert not set(g64) & set(M.BUFFERS)
    save(name, {**common(arch, sd, sd_seed, inp, obj_num), "G": G, "out": o64, "loss": np.float64(l64), **compact(g64), **gates(g32, g64, o32, o64, l32, l64)})


# ---- the diffusion objective ----
def objective_inputs(arch, sd_seed, in_seed, B, T, mask_len, steps):
    """weights, conditioning, x_start, mask, loss weights, and per step t (B,) and noise (B, F, 1, T)"""
    sd = M.seeded_state_dict(arch, sd_seed)
    inp, _ = M.seeded_inputs(arch, B, T, 2, in_seed)
    rng = np.random.default_rng(in_seed + 1)
    inp["x_start"] = rng.normal(0, 0.5, (B, arch.input_dim, 1, T)).astype(np.float32)
    inp["mask"] = np.arange(T)[None, :] < np.asarray(mask_len)[:, None]
    inp["weights"] = np.ones(B, np.float32)
    ts = rng.integers(0, 1000, (steps, B)).astype(np.int64)
    noise = rng.normal(size=(steps, B, arch.input_dim, 1, T)).astype(np.float32)
    return sd, inp, ts, noise


def objective(model, diffusion, inp, t, noise, dtype):
    """-> (the reference's terms, (terms["loss"] * weights).mean())"""
    batch = batch_of(model, inp, dtype)
    terms, _ = diffusion.training_losses(model, torch.from_numpy(inp["x_start"]).to(dtype), torch.from_numpy(t), model_kwargs={"batch": batch},
                                         noise=torch.from_numpy(noise).to(dtype))
    return terms, (terms["loss"] * torch.from_numpy(inp["weights"]).to(dtype)).mean()


def losses_run(Model, diffusion, arch, sd, inp, t, noise, dtype):
    model = build(Model, arch, sd, dtype)
    terms, loss = objective(model, diffusion, inp, t, noise, dtype)
    loss.backward()
    x_t = diffusion.q_sample(torch.from_numpy(inp["x_start"]).to(dtype), torch.from_numpy(t), noise=torch.from_numpy(noise).to(dtype))
    return x_t.double().numpy(), terms["mse"].detach().double().numpy(), float(loss.detach()), named_grads(model)


def capture_losses(Model, diffusion, name, arch, sd_seed, in_seed):
    sd, inp, ts, noise = objective_inputs(arch, sd_seed, in_seed, 3, 12, (12, 7, 1), 1)
    inp["t"] = ts[0]
    x64, m64, l64, g64 = losses_run(Model, diffusion, arch, sd, inp, ts[0], noise[0], torch.float64)
    x32, m32, l32, g32 = losses_run(Model, diffusion, arch, sd, inp, ts[0], noise[0], torch.float32)
    e_mse, e_xt = rel(m32, m64), max(rel(x32, x64), 2.0 ** -24)
    save(name, {**common(arch, sd, sd_seed, inp, None), "in/x_start": inp["x_start"], "in/mask": inp["mask"], "in/weights": inp["weights"],
                "in/noise": noise[0], "diffusion_steps": np.int32(1000), "x_t": x64, "mse": m64, "out": m64, "loss": np.float64(l64),
                "e32_mse": np.float64(e_mse), "tol_rel_mse": np.float64(4 * e_mse), "e32_x_t": np.float64(e_xt), "tol_rel_x_t": np.float64(4 * e_xt),
                **compact(g64), **gates(g32, g64, m32, m64, l32, l64)})


def sgd_run(Model, diffusion, arch, sd, inp, ts, noise, dtype):
    model = build(Model, arch, sd, dtype)
    opt = torch.optim.SGD(model.parameters(), lr=SGD_LR)
    curve = []
    for k in range(SGD_STEPS):
        opt.zero_grad()
        _, loss = objective(model, diffusion, inp, ts[k], noise[k], dtype)
        loss.backward()
        opt.step()
        curve.append(float(loss.detach()))
    return np.array(curve)


def capture_sgd(Model, diffusion, name, arch, sd_seed, in_seed):
    sd, inp, ts, noise = objective_inputs(arch, sd_seed, in_seed, 3, 12, (12, 7, 1), SGD_STEPS)
    inp["t"] = ts
    c64 = sgd_run(Model, diffusion, arch, sd, inp, ts, noise, torch.float64)
    c32 = sgd_run(Model, diffusion, arch, sd, inp, ts, noise, torch.float32)
    data = {**common(arch, sd, sd_seed, inp, None), "in/x_start": inp["x_start"], "in/mask": inp["mask"], "in/weights": inp["weights"],
            "in/noise": noise, "diffusion_steps": np.int32(1000), "lr": np.float64(SGD_LR), "curve": c64, "curve32": c32}
    path = os.path.join(GOLDEN, name)
    np.savez_compressed(path, **data)
    print(f"{name}: float64 curve {c64}; float32 deviation {np.abs(c32 - c64).max():.3e}; {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1000000


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.join(sys.argv[1], "src"))
    install_clip_stand_in()
    from oakink2_tamf.model.diffusion_util import create_gaussian_diffusion
    from oakink2_tamf.model.interaction_segment_mdm import InterationSegmentMDM as Model

    capture_trunk(Model, "mdmtrain_l1_hd64.npz", M.ARCH_L1_64, 301, 302, B=2, T=1, nobj=2, ragged=False)
    capture_trunk(Model, "mdmtrain_l1_hd128.npz", M.ARCH_L1_128, 311, 312, B=2, T=1, nobj=2, ragged=False)
    capture_trunk(Model, "mdmtrain_tiny_hd64.npz", M.ARCH_TINY_64, 321, 322, B=3, T=12, nobj=2, ragged=True, mask_len=(12, 7, 1))
    capture_trunk(Model, "mdmtrain_tiny_hd128.npz", M.ARCH_TINY_128, 331, 332, B=3, T=12, nobj=2, ragged=True, mask_len=(12, 7, 1))
    diffusion = create_gaussian_diffusion(1000, "cosine")
    capture_losses(Model, diffusion, "mdmtrain_losses.npz", M.ARCH_TINY_128, 341, 342)
    capture_sgd(Model, diffusion, "mdmtrain_sgd.npz", M.ARCH_TINY_128, 351, 352)


if __name__ == "__main__":
    main()
