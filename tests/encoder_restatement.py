"""Float64 restatement of the SegmentEncoder forward (reference model/segment_encoder.py:77-111) in plain torch, written from its
semantics: the GPU tests compare the HIP encoder against it where the reference itself is not importable.  It is pinned on the
reference by tests/test_encoder_cpu.py (every tests/golden/segment_encoder_*.npz fixture to 1e-5).

obj_num=None averages the object rows over the whole (padded) object axis, as the reference's forward on the batch it is given; a
per-clip count averages over each clip's own objects (the FID script's batches of one clip)."""
from __future__ import annotations

import math
from typing import Dict, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

ARCH_ENCODER = dict(input_dim=99, obj_input_dim=9, hand_shape_dim=10, obj_embed_dim=768, latent_dim=64, ff_size=128, num_layers=2,
                    num_heads=4)  # config/arch_encoder.yml


def _t(v) -> torch.Tensor:
    return torch.as_tensor(np.asarray(v)).to(torch.float64)


def _lin(sd, name, x):
    return x @ _t(sd[name + ".weight"]).T + _t(sd[name + ".bias"])


def _silu(x):
    return x / (1.0 + torch.exp(-x))


def _layer_norm(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def _object_mean(x: torch.Tensor, obj_num: Optional[Sequence[int]]) -> torch.Tensor:
    """mean over axis 1 (objects) of (B, nobj, ...): all rows, or each clip's first obj_num[b]"""
    if obj_num is None:
        return x.mean(1)
    return torch.stack([x[b, : int(n)].mean(0) for b, n in enumerate(obj_num)], 0)


def encoder_forward(sd: Mapping[str, np.ndarray], arch: Mapping[str, int], pose_repr, shape, hand_side, obj_embedding, obj_traj,
                    obj_num: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """-> (encoding (B, d), activation (B, input_dim)), float64.  hand_side: B x ("rh" | "lh" | 0 | 1)."""
    d, H, L = int(arch["latent_dim"]), int(arch["num_heads"]), int(arch["num_layers"])
    hd = d // H
    pose, shp, oemb, otraj = _t(pose_repr), _t(shape), _t(obj_embedding), _t(obj_traj)
    B, T, _ = pose.shape
    nan_to_num = torch.nan_to_num
    # three prefix rows
    side = torch.stack([_t(sd["hand_side_process.lh_embed"] if s in ("lh", 1, b"lh") else sd["hand_side_process.rh_embed"])
                        for s in hand_side], 0)
    row_shape = _lin(sd, "hand_shape_process.shape_embed", shp.mean(1))
    row_obj = _lin(sd, "obj_embed_process.embedding", _object_mean(oemb, obj_num))
    prefix = nan_to_num(torch.stack([side, row_shape, row_obj], 1))  # (B, 3, d)
    # frame rows: the object trajectory embedded per object, then averaged
    hand = _lin(sd, "input_process.poseEmbedding", pose)                          # (B, T, d)
    objs = _object_mean(_lin(sd, "obj_input_process.poseEmbedding", otraj), obj_num)  # (B, T, d)
    z = _silu(_lin(sd, "input_merge.0", torch.cat([hand, objs], -1)))
    frames = nan_to_num(_lin(sd, "input_merge.2", z))
    cls = _t(sd["classification_token"]).reshape(1, 1, d).expand(B, 1, d)
    x = torch.cat([prefix, frames, cls], 1)                                       # (B, T + 4, d)
    S = x.shape[1]
    x = x + _t(sd["sequence_pos_encoder.pe"])[:S, 0][None]
    for l in range(L):
        p = f"seqTransEncoder.layers.{l}."
        qkv = x @ _t(sd[p + "self_attn.in_proj_weight"]).T + _t(sd[p + "self_attn.in_proj_bias"])
        q, k, v = (qkv[..., i * d:(i + 1) * d].reshape(B, S, H, hd).transpose(1, 2) for i in range(3))
        att = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), -1) @ v      # no mask: every row attends to every row
        att = att.transpose(1, 2).reshape(B, S, d)
        x = _layer_norm(x + _lin(sd, p + "self_attn.out_proj", att), _t(sd[p + "norm1.weight"]), _t(sd[p + "norm1.bias"]))
        hid = _lin(sd, p + "linear1", x)
        hid = 0.5 * hid * (1.0 + torch.erf(hid / math.sqrt(2.0)))
        x = _layer_norm(x + _lin(sd, p + "linear2", hid), _t(sd[p + "norm2.weight"]), _t(sd[p + "norm2.bias"]))
    enc = x[:, -1]
    a = _silu(_lin(sd, "output_process.poseFinal.0", enc))
    a = _silu(_lin(sd, "output_process.poseFinal.2", a))
    act = _lin(sd, "output_process.poseFinal.4", a)
    return enc.numpy(), act.numpy()


def seeded_state_dict(arch: Mapping[str, int], seed: int, scale: float = 1.0) -> Dict[str, np.ndarray]:
    """float32 weights with the encoder's key set (PyTorch-like uniform fan-in init, LayerNorm gains around 1, the reference's
    sin/cos PE table and hand-side buffers), deterministic in `seed`"""
    rng = np.random.default_rng(seed)
    d, ff, F = int(arch["latent_dim"]), int(arch["ff_size"]), int(arch["input_dim"])
    sd: Dict[str, np.ndarray] = {}

    def lin(name, o, i):
        bound = scale / math.sqrt(i)
        sd[name + ".weight"] = rng.uniform(-bound, bound, (o, i)).astype(np.float32)
        sd[name + ".bias"] = rng.uniform(-bound, bound, (o,)).astype(np.float32)

    sd["hand_side_process.rh_embed"] = np.zeros(d, np.float32)
    lh = np.zeros(d, np.float32)
    lh[0] = 1.0
    sd["hand_side_process.lh_embed"] = lh
    lin("hand_shape_process.shape_embed", d, int(arch["hand_shape_dim"]))
    lin("obj_embed_process.embedding", d, int(arch["obj_embed_dim"]))
    sd["classification_token"] = rng.normal(0, 0.5, (1, 1, d)).astype(np.float32)
    lin("input_process.poseEmbedding", d, F)
    lin("obj_input_process.poseEmbedding", d, int(arch["obj_input_dim"]))
    lin("input_merge.0", d, 2 * d)
    lin("input_merge.2", d, d)
    sd["sequence_pos_encoder.pe"] = pe_table(d)
    for l in range(int(arch["num_layers"])):
        p = f"seqTransEncoder.layers.{l}."
        bound = scale / math.sqrt(d)
        sd[p + "self_attn.in_proj_weight"] = rng.uniform(-bound, bound, (3 * d, d)).astype(np.float32)
        sd[p + "self_attn.in_proj_bias"] = rng.uniform(-bound, bound, (3 * d,)).astype(np.float32)
        lin(p + "self_attn.out_proj", d, d)
        lin(p + "linear1", ff, d)
        lin(p + "linear2", d, ff)
        for n in ("norm1", "norm2"):
            sd[p + n + ".weight"] = (1.0 + 0.1 * rng.normal(size=d)).astype(np.float32)
            sd[p + n + ".bias"] = (0.1 * rng.normal(size=d)).astype(np.float32)
    lin("output_process.poseFinal.0", d, d)
    lin("output_process.poseFinal.2", d, d)
    lin("output_process.poseFinal.4", F, d)
    return sd


def seeded_inputs(B: int, T: int, nobj: int, seed: int, obj_num: Optional[Sequence[int]] = None, arch=ARCH_ENCODER) -> Dict:
    """a batch shaped like the collate's: pose_repr (B,T,99), shape (B,T,10), hand_side, obj_embedding (B,nobj,768), obj_traj
    (B,nobj,T,9); rows past a clip's obj_num are zero (the collate's padding)"""
    rng = np.random.default_rng(seed)
    F, sdim, od, qd = int(arch["input_dim"]), int(arch["hand_shape_dim"]), int(arch["obj_embed_dim"]), int(arch["obj_input_dim"])
    out = {
        "pose_repr": rng.normal(0, 0.5, (B, T, F)).astype(np.float32),
        "shape": np.repeat(rng.normal(0, 1.0, (B, 1, sdim)), T, axis=1).astype(np.float32),
        "hand_side": ["lh" if rng.random() < 0.5 else "rh" for _ in range(B)],
        "obj_embedding": rng.normal(0, 0.2, (B, nobj, od)).astype(np.float32),
        "obj_traj": rng.normal(0, 0.5, (B, nobj, T, qd)).astype(np.float32),
    }
    if obj_num is not None:
        for b, n in enumerate(obj_num):
            out["obj_embedding"][b, int(n):] = 0.0
            out["obj_traj"][b, int(n):] = 0.0
    return out


def pe_table(d: int, rows: int = 5000) -> np.ndarray:
    """the (rows, 1, d) float32 sin/cos table of PositionalEncoding (the `sequence_pos_encoder.pe` buffer)"""
    from oakink2_tamf_amd.model.interaction_segment_mdm import PositionalEncoding

    return PositionalEncoding(d, max_len=rows).pe.numpy()


def load_encoder_case(path: str) -> Dict:
    """a tests/golden/segment_encoder_*.npz fixture -> {"sd", "arch", "inputs", "out", "keys"}; the PE table is rebuilt, its first
    rows replaced by the ones the fixture stores"""
    z = np.load(path, allow_pickle=False)
    names = ("input_dim", "obj_input_dim", "hand_shape_dim", "obj_embed_dim", "latent_dim", "ff_size", "num_layers", "num_heads")
    arch = dict(zip(names, (int(v) for v in z["arch"])))
    sd = {k[3:]: z[k] for k in z.files if k.startswith("sd/")}
    pe = pe_table(arch["latent_dim"])
    head = z["pe_head"]  # the rows a forward reads (S <= 256), as the reference had them: libm's sin / cos differ by ulps across hosts
    assert np.abs(pe[: head.shape[0], 0] - head).max() <= 1e-5, "rebuilt PE table differs from the fixture's rows"
    pe[: head.shape[0], 0] = head
    sd["sequence_pos_encoder.pe"] = pe
    inputs = {k[3:]: z[k] for k in z.files if k.startswith("in/")}
    inputs["hand_side"] = [str(s) for s in inputs["hand_side"]]
    out = {k[4:]: z[k] for k in z.files if k.startswith("out/")}
    return {"sd": sd, "arch": arch, "inputs": inputs, "out": out, "keys": [str(k) for k in z["state_dict_keys"]]}
