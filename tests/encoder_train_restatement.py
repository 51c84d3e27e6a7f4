"""Float64 restatement of the SegmentEncoder TRAINING forward and its loss in plain torch with autograd, written from the semantics
(reference model/segment_encoder.py:77-111 under train(), model/segment_encoder_loss.py; the dropout sites by the published
definitions of PositionalEncoding and nn.TransformerEncoderLayer), with injectable keep-masks per dropout site.  Pinned on the
reference's own module and loss by tests/test_enctrain_cpu.py (every tests/golden/enctrain_*.npz fixture, dropout off).

Sites (include/tamf_enctrain.h): 0 the sum x + PE (S, 64); per layer l: 1 + 4l attention probabilities (4 S, S) head-major,
2 + 4l out-projection output (S, 64), 3 + 4l GELU output (S, ff), 4 + 4l linear2 output (S, 64).
masks: {site: bool (B, rows, cols)}; a site without a mask keeps everything (and is not scaled)."""
from __future__ import annotations

import hashlib
import math
from typing import Dict, Mapping, Optional, Sequence

import numpy as np
import torch

from encoder_restatement import _layer_norm, _object_mean, _silu, pe_table, seeded_state_dict

BUFFERS = ("classification_token", "hand_side_process.rh_embed", "hand_side_process.lh_embed", "sequence_pos_encoder.pe")
ARCH_NAMES = ("input_dim", "obj_input_dim", "hand_shape_dim", "obj_embed_dim", "latent_dim", "ff_size", "num_layers", "num_heads")


def leaf_state_dict(sd: Mapping[str, np.ndarray], dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """float64 (or `dtype`) tensors; every trainable one a leaf that requires grad"""
    out = {}
    for k, v in sd.items():
        t = torch.as_tensor(np.asarray(v)).to(dtype).clone()
        out[k] = t.requires_grad_(k not in BUFFERS)
    return out


def _lin(sd, name, x):
    return x @ sd[name + ".weight"].T + sd[name + ".bias"]


def _drop(x, masks, site, p, view=None):
    if masks is None or site not in masks or p == 0.0:
        return x
    m = torch.as_tensor(np.asarray(masks[site])).to(x.dtype)
    if view is not None:
        m = m.reshape(view)
    return x * m / (1.0 - p)


def train_forward(sd: Mapping[str, torch.Tensor], arch: Mapping[str, int], inputs: Mapping, labels, obj_num: Optional[Sequence[int]] = None,
                  masks: Optional[Mapping[int, np.ndarray]] = None, p: float = 0.0):
    """-> (loss, activation (B, input_dim)) as torch tensors of the dtype of `sd`, attached to its leaves"""
    d, H, L = int(arch["latent_dim"]), int(arch["num_heads"]), int(arch["num_layers"])
    hd = d // H
    dtype = sd["input_merge.0.weight"].dtype
    f64 = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)  # noqa: E731
    pose, shp, oemb, otraj = f64(inputs["pose_repr"]), f64(inputs["shape"]), f64(inputs["obj_embedding"]), f64(inputs["obj_traj"])
    B, T, _ = pose.shape
    side = torch.stack([sd["hand_side_process.lh_embed"] if s in ("lh", 1, b"lh") else sd["hand_side_process.rh_embed"]
                        for s in inputs["hand_side"]], 0)
    row_shape = _lin(sd, "hand_shape_process.shape_embed", shp.mean(1))
    row_obj = _object_mean(_lin(sd, "obj_embed_process.embedding", oemb), obj_num)     # embedded per object, then averaged
    prefix = torch.nan_to_num(torch.stack([side, row_shape, row_obj], 1))
    hand = _lin(sd, "input_process.poseEmbedding", pose)
    objs = _object_mean(_lin(sd, "obj_input_process.poseEmbedding", otraj), obj_num)
    z = _silu(_lin(sd, "input_merge.0", torch.cat([hand, objs], -1)))
    frames = torch.nan_to_num(_lin(sd, "input_merge.2", z))
    cls = sd["classification_token"].reshape(1, 1, d).expand(B, 1, d)
    x = torch.cat([prefix, frames, cls], 1)
    S = x.shape[1]
    x = _drop(x + sd["sequence_pos_encoder.pe"][:S, 0][None], masks, 0, p)
    for l in range(L):
        k_ = f"seqTransEncoder.layers.{l}."
        site = 1 + 4 * l
        qkv = x @ sd[k_ + "self_attn.in_proj_weight"].T + sd[k_ + "self_attn.in_proj_bias"]
        q, k, v = (qkv[..., i * d:(i + 1) * d].reshape(B, S, H, hd).transpose(1, 2) for i in range(3))
        prob = _drop(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), -1), masks, site, p, view=(B, H, S, S))
        att = (prob @ v).transpose(1, 2).reshape(B, S, d)
        x = _layer_norm(x + _drop(_lin(sd, k_ + "self_attn.out_proj", att), masks, site + 1, p), sd[k_ + "norm1.weight"], sd[k_ + "norm1.bias"])
        hid = _lin(sd, k_ + "linear1", x)
        hid = _drop(0.5 * hid * (1.0 + torch.erf(hid / math.sqrt(2.0))), masks, site + 2, p)
        x = _layer_norm(x + _drop(_lin(sd, k_ + "linear2", hid), masks, site + 3, p), sd[k_ + "norm2.weight"], sd[k_ + "norm2.bias"])
    a = _silu(_lin(sd, "output_process.poseFinal.0", x[:, -1]))
    a = _silu(_lin(sd, "output_process.poseFinal.2", a))
    act = _lin(sd, "output_process.poseFinal.4", a)
    lab = torch.as_tensor(np.asarray(labels)).long()
    logp = act - torch.logsumexp(act, -1, keepdim=True)
    loss = -logp[torch.arange(B), lab].mean()
    return loss, act


def loss_and_grads(sd_np: Mapping[str, np.ndarray], arch, inputs, labels, obj_num=None, masks=None, p: float = 0.0, dtype=torch.float64):
    """-> (loss float, activation (B, F) float64, {key: gradient float64} for every trainable key), computed in `dtype`"""
    sd = leaf_state_dict(sd_np, dtype)
    loss, act = train_forward(sd, arch, inputs, labels, obj_num, masks, p)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy() for k, v in sd.items() if k not in BUFFERS}
    return float(loss.detach()), act.detach().double().numpy(), grads


def grad_rel_err(got: Mapping[str, np.ndarray], ref: Mapping[str, np.ndarray]) -> Dict[str, float]:
    """{key: |got - ref|_inf / |ref|_inf} over the finite entries of ref; NaN entries have to be NaN in both (inf when they are not)"""
    out = {}
    for k, r in ref.items():
        r, g = np.asarray(r, np.float64), np.asarray(got[k], np.float64)
        nan = np.isnan(r)
        if (np.isnan(g) != nan).any():
            out[k] = float("inf")
        elif nan.all() or np.nanmax(np.abs(r)) == 0:
            out[k] = 0.0 if nan.all() else float(np.nanmax(np.abs(g - r)))
        else:
            out[k] = float(np.nanmax(np.abs(g - r)) / np.nanmax(np.abs(r)))
    return out


def site_shapes(arch, T: int) -> Dict[int, tuple]:
    """{site: (rows, cols)} of every dropout site of a clip of T frames"""
    S, d, ff, H = T + 4, int(arch["latent_dim"]), int(arch["ff_size"]), int(arch["num_heads"])
    out = {0: (S, d)}
    for l in range(int(arch["num_layers"])):
        out.update({1 + 4 * l: (H * S, S), 2 + 4 * l: (S, d), 3 + 4 * l: (S, ff), 4 + 4 * l: (S, d)})
    return out


def sd_digest(sd: Mapping[str, np.ndarray]) -> str:
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()


def load_train_case(path: str) -> Dict:
    """a tests/golden/enctrain_*.npz fixture -> {"sd", "arch", "inputs", "labels", "obj_num", "loss", "grads", "tol_rel", "tol_rel_loss"}
    (+ "sgd_*" where stored).  Weights are stored, or regenerated from `sd_seed` and checked against `sd_sha256`; the PE table is
    rebuilt with its first rows replaced by the stored ones."""
    z = np.load(path, allow_pickle=False)
    arch = dict(zip(ARCH_NAMES, (int(v) for v in z["arch"])))
    if "sd_seed" in z.files:
        sd = seeded_state_dict(arch, int(z["sd_seed"]))
        del sd["sequence_pos_encoder.pe"]
        assert sd_digest(sd) == str(z["sd_sha256"]), "the regenerated weights differ from the ones the fixture was captured with"
    else:
        sd = {k[3:]: z[k] for k in z.files if k.startswith("sd/")}
    pe = pe_table(arch["latent_dim"])
    head = z["pe_head"]
    assert np.abs(pe[: head.shape[0], 0] - head).max() <= 1e-5, "rebuilt PE table differs from the fixture's rows"
    pe[: head.shape[0], 0] = head
    sd["sequence_pos_encoder.pe"] = pe
    inputs = {k[3:]: z[k] for k in z.files if k.startswith("in/") and k != "in/obj_num"}
    inputs["hand_side"] = [str(s) for s in inputs["hand_side"]]
    out = {"sd": sd, "arch": arch, "inputs": inputs, "labels": z["labels"], "obj_num": [int(v) for v in z["in/obj_num"]] if "in/obj_num" in z.files else None,
           "loss": float(z["loss"]), "grads": {k[5:]: z[k] for k in z.files if k.startswith("grad/")}, "tol_rel": float(z["tol_rel"]),
           "tol_rel_loss": float(z["tol_rel_loss"])}
    for k in z.files:
        if k.startswith("sgd_"):
            out[k] = z[k]
    return out
