"""Seeded inputs of the point-encoder tests: weights with the key set of the reference's PointTransformer (without the
`module.point_encoder.` prefix), point clouds, and a plain-torch restatement of the encoder on given groups (any dtype), written from
the semantics of reference model/pointbert/point_encoder.py:163-183 and dvae.py:150-221.  Weights are regenerated at test time and
never stored (the full model has 21.9 M parameters); tools/capture_pointenc_golden.py records their checksum beside the reference's
outputs, so a fixture and the weights it was captured with cannot drift apart unnoticed.

SWEEP: configurations at the edges of what tamf_pointenc_model_create accepts, with seeded weights and clouds of their own and the
float64 / float32 restatement as their reference (tests/test_pointenc_edges_gpu.py).  host_fps / host_knn: include/tamf_pointenc.h's
selection rules in float32 numpy - the same expression with every product and sum rounded on its own, so they are exact references."""
from __future__ import annotations

import hashlib
import math
from typing import Dict, Mapping, Tuple

import numpy as np
import torch

# case -> (cfg of HipPointEncoder, points per cloud, clouds); token counts 18, 65, 513: none a multiple of 16
CASES = {
    "tiny": (dict(point_dims=3, trans_dim=128, depth=2, num_heads=2, num_group=17, group_size=8, encoder_dims=64), 250, 3),
    "mid": (dict(point_dims=6, trans_dim=384, depth=2, num_heads=6, num_group=64, group_size=32, encoder_dims=256), 1024, 2),
    "full": (dict(point_dims=6, trans_dim=384, depth=12, num_heads=6, num_group=512, group_size=32, encoder_dims=256), 8192, 2),
}
WEIGHT_SEED = {"tiny": 101, "mid": 102, "full": 103}


def _cfg(C, D, depth, G, M, E):
    return dict(point_dims=C, trans_dim=D, depth=depth, num_heads=D // 64, num_group=G, group_size=M, encoder_dims=E)


# case -> (cfg, points per cloud, clouds).  T = num_group + 1 tokens, Tp = round_up(T, 4); the attention kernel's dynamic LDS is
# 64 * pe_att_ts(T) + 64 bytes, above 64 KiB from T = 993 on.
SWEEP = {
    "low": (_cfg(3, 64, 1, 1, 8, 16), 8, 1),          # T = 2 (empty pooling loop), group_size = N, E = 16 (column and K tails)
    "odd": (_cfg(3, 64, 2, 15, 9, 48), 100, 5),       # T = 16 (one full query panel), tails of 48, group rows of 9, batch of 4 + 1
    "t24": (_cfg(6, 128, 1, 23, 33, 80), 120, 2),     # Tp = T = 24: the P.V loop has no tail step and no padded column
    "t23": (_cfg(6, 128, 1, 22, 63, 16), 120, 2),     # Tp - T = 1
    "wideE": (_cfg(6, 128, 1, 16, 64, 1024), 200, 2),  # T = 17 (a panel with one live row), the widest encoder_dims, group_size 64
    "wideD": (_cfg(3, 1024, 1, 17, 8, 64), 150, 1),   # trans_dim 1024: 3072 and 4096 columns, 16 heads
    "g991": (_cfg(3, 64, 1, 991, 8, 16), 1100, 1),    # T = 992: the last below 64 KiB of attention LDS
    "g992": (_cfg(3, 64, 1, 992, 8, 16), 1100, 1),    # T = 993: the first above
    "g1024": (_cfg(3, 128, 2, 1024, 8, 16), 1100, 2),  # the upper limit, Tp - T = 3
}
SWEEP_SEED = {name: 200 + i for i, name in enumerate(SWEEP)}  # weights: seed, clouds: seed + 100, centres: seed + 200


def seeded_state_dict(cfg: Mapping[str, int], seed: int) -> Dict[str, np.ndarray]:
    """float32 weights, deterministic in `seed`: linear maps uniform in +-1/sqrt(fan_in) (biases too), BatchNorm with non-trivial
    affine parameters and running statistics, LayerNorm gains around 1 with offsets, cls_token / cls_pos normal"""
    rng = np.random.default_rng(seed)
    C, D, E = int(cfg["point_dims"]), int(cfg["trans_dim"]), int(cfg["encoder_dims"])
    sd: Dict[str, np.ndarray] = {}

    def lin(name, o, i, conv=False, bias=True):
        bound = 1.0 / math.sqrt(i)
        sd[name + ".weight"] = rng.uniform(-bound, bound, (o, i, 1) if conv else (o, i)).astype(np.float32)
        if bias:
            sd[name + ".bias"] = rng.uniform(-bound, bound, (o,)).astype(np.float32)

    def bn(name, n):
        sd[name + ".weight"] = (1.0 + 0.2 * rng.normal(size=n)).astype(np.float32)
        sd[name + ".bias"] = (0.1 * rng.normal(size=n)).astype(np.float32)
        sd[name + ".running_mean"] = (0.1 * rng.normal(size=n)).astype(np.float32)
        sd[name + ".running_var"] = rng.uniform(0.05, 0.5, n).astype(np.float32)

    def ln(name):
        sd[name + ".weight"] = (1.0 + 0.1 * rng.normal(size=D)).astype(np.float32)
        sd[name + ".bias"] = (0.1 * rng.normal(size=D)).astype(np.float32)

    lin("encoder.first_conv.0", 128, C, conv=True)
    bn("encoder.first_conv.1", 128)
    lin("encoder.first_conv.3", 256, 128, conv=True)
    lin("encoder.second_conv.0", 512, 512, conv=True)
    bn("encoder.second_conv.1", 512)
    lin("encoder.second_conv.3", E, 512, conv=True)
    lin("reduce_dim", D, E)
    sd["cls_token"] = rng.normal(0, 0.5, (1, 1, D)).astype(np.float32)
    sd["cls_pos"] = rng.normal(0, 1.0, (1, 1, D)).astype(np.float32)
    lin("pos_embed.0", 128, 3)
    lin("pos_embed.2", D, 128)
    for l in range(int(cfg["depth"])):
        p = f"blocks.blocks.{l}."
        ln(p + "norm1")
        ln(p + "norm2")
        lin(p + "mlp.fc1", 4 * D, D)
        lin(p + "mlp.fc2", D, 4 * D)
        lin(p + "attn.qkv", 3 * D, D, bias=False)
        lin(p + "attn.proj", D, D)
    ln("norm")
    return sd


def state_checksum(sd: Mapping[str, np.ndarray]) -> str:
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k], dtype=np.float32).tobytes())
    return h.hexdigest()


def seeded_clouds(B: int, N: int, C: int, seed: int) -> np.ndarray:
    """(B, N, C) float32: points uniform in a box of about 0.2 m (an object's size) off the origin, colours uniform in [0, 1)"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-0.1, 0.1, (B, N, 3)) * np.array([1.0, 0.7, 1.3]) + np.array([0.02, -0.01, 0.03])
    rest = rng.uniform(0.0, 1.0, (B, N, C - 3))
    return np.concatenate([xyz, rest], -1).astype(np.float32)


def _layer_norm(x, g, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * g + b


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def pointnet_first_layer(sd, x, dtype=torch.float64):
    """relu(BatchNorm1d(Conv1d(x))) of encoder.first_conv, unfolded, eval mode: x (..., C) -> (..., 128)"""
    t = lambda k: torch.as_tensor(np.asarray(sd[k])).to(dtype)  # noqa: E731
    h = torch.as_tensor(x).to(dtype) @ t("encoder.first_conv.0.weight")[:, :, 0].T + t("encoder.first_conv.0.bias")
    h = (h - t("encoder.first_conv.1.running_mean")) / torch.sqrt(t("encoder.first_conv.1.running_var") + 1e-5)
    return torch.relu(h * t("encoder.first_conv.1.weight") + t("encoder.first_conv.1.bias"))


def restatement(sd: Mapping[str, np.ndarray], cfg: Mapping[str, int], points, centre_idx, nbr_idx, dtype=torch.float64, device="cpu"):
    """the encoder on given groups in plain torch: points (B, N, C), centre_idx (B, G), nbr_idx (B, G, M) -> (B, 2 * trans_dim)"""
    def t(k):  # (arrays, or tensors already on the device)
        v = sd[k]
        return (v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))).to(device=device, dtype=dtype)

    D, H = int(cfg["trans_dim"]), int(cfg["num_heads"])
    p = torch.as_tensor(points).to(device=device, dtype=dtype)
    ci, ni = torch.as_tensor(centre_idx).to(device).long(), torch.as_tensor(nbr_idx).to(device).long()
    B, G, M = ni.shape
    bi = torch.arange(B, device=device)
    centre = p[bi[:, None], ci][..., :3]                      # (B, G, 3)
    nb = p[bi[:, None, None], ni].clone()                     # (B, G, M, C)
    nb[..., :3] -= centre[:, :, None]

    def bn(x, name):
        return (x - t(name + ".running_mean")) / torch.sqrt(t(name + ".running_var") + 1e-5) * t(name + ".weight") + t(name + ".bias")

    def conv(x, name):
        return x @ t(name + ".weight")[:, :, 0].T + t(name + ".bias")

    f = conv(torch.relu(bn(conv(nb, "encoder.first_conv.0"), "encoder.first_conv.1")), "encoder.first_conv.3")  # (B, G, M, 256)
    f = torch.cat([f.max(2, keepdim=True)[0].expand(-1, -1, M, -1), f], -1)
    f = conv(torch.relu(bn(conv(f, "encoder.second_conv.0"), "encoder.second_conv.1")), "encoder.second_conv.3")
    tok = f.max(2)[0] @ t("reduce_dim.weight").T + t("reduce_dim.bias")
    pos = _gelu(centre @ t("pos_embed.0.weight").T + t("pos_embed.0.bias")) @ t("pos_embed.2.weight").T + t("pos_embed.2.bias")
    x = torch.cat([t("cls_token").expand(B, -1, -1), tok], 1)
    pos = torch.cat([t("cls_pos").expand(B, -1, -1), pos], 1)
    T = G + 1
    for l in range(int(cfg["depth"])):
        k = f"blocks.blocks.{l}."
        x = x + pos
        qkv = (_layer_norm(x, t(k + "norm1.weight"), t(k + "norm1.bias")) @ t(k + "attn.qkv.weight").T).reshape(B, T, 3, H, D // H).permute(2, 0, 3, 1, 4)
        att = torch.softmax(qkv[0] @ qkv[1].transpose(-2, -1) * (D // H) ** -0.5, -1)
        x = x + (att @ qkv[2]).transpose(1, 2).reshape(B, T, D) @ t(k + "attn.proj.weight").T + t(k + "attn.proj.bias")
        h = _gelu(_layer_norm(x, t(k + "norm2.weight"), t(k + "norm2.bias")) @ t(k + "mlp.fc1.weight").T + t(k + "mlp.fc1.bias"))
        x = x + h @ t(k + "mlp.fc2.weight").T + t(k + "mlp.fc2.bias")
    x = _layer_norm(x, t("norm.weight"), t("norm.bias"))
    return torch.cat([x[:, 0], x[:, 1:].max(1)[0]], -1)


def host_fps(xyz: np.ndarray, G: int, start: int) -> Tuple[np.ndarray, float]:
    """tamf_pointenc_fps on the host for one cloud xyz (N, >= 3) float32: ((dx*dx + dy*dy) + dz*dz) with every product and sum
    rounded to float32 on its own, the running minimum from 1e10, argmax to the lowest index among equals.  -> (indices (G,) int64,
    the smallest relative gap between the two largest running minima over the steps; 0 where they are equal, inf for N = 1)"""
    xyz = np.ascontiguousarray(np.asarray(xyz)[:, :3], dtype=np.float32)
    N = xyz.shape[0]
    d, far, idx, gap = np.full(N, np.float32(1e10)), int(start), [], np.inf
    for _ in range(G):
        idx.append(far)
        diff = xyz - xyz[far]
        d = np.minimum(d, (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2])
        if N > 1:
            top = np.partition(d, N - 2)[-2:]
            gap = min(gap, float((top[1] - top[0]) / top[1]) if top[1] > 0 else 0.0)
        far = int(np.argmax(d))
    return np.asarray(idx, dtype=np.int64), gap


def host_knn(xyz: np.ndarray, centre_idx, M: int) -> np.ndarray:
    """tamf_pointenc_group on the host for one cloud: the M nearest points of each centre by the same float32 expression, in
    ascending (distance, index) order.  xyz (N, >= 3) float32, centre_idx (G,) -> (G, M) int64"""
    xyz = np.ascontiguousarray(np.asarray(xyz)[:, :3], dtype=np.float32)
    index = np.arange(xyz.shape[0])
    out = []
    for c in np.asarray(centre_idx).reshape(-1):
        diff = xyz - xyz[int(c)]
        d = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
        out.append(np.lexsort((index, d))[:M])
    return np.asarray(out, dtype=np.int64)


def drawn_groups(points: np.ndarray, G: int, M: int, seed: int):
    """centres drawn without replacement and their host_knn neighbours: points (B, N, C) -> (centre_idx (B, G), nbr_idx (B, G, M))"""
    rng = np.random.default_rng(seed)
    centre = np.stack([rng.choice(points.shape[1], G, replace=False) for _ in range(points.shape[0])]).astype(np.int64)
    return centre, np.stack([host_knn(points[b], centre[b], M) for b in range(points.shape[0])])


_SWEEP_CACHE: Dict[str, dict] = {}


def sweep_case(name: str) -> dict:
    """inputs and reference of one SWEEP case, computed once and shared (do not modify): cfg, sd, points, centre_idx, nbr_idx, out64
    (the float64 restatement) and e32 = max |float32 restatement - float64 restatement|, the unit of the project's 4 * e32 gate"""
    if name not in _SWEEP_CACHE:
        cfg, N, B = SWEEP[name]
        seed = SWEEP_SEED[name]
        sd = seeded_state_dict(cfg, seed)
        points = seeded_clouds(B, N, cfg["point_dims"], seed + 100)
        centre, nbr = drawn_groups(points, cfg["num_group"], cfg["group_size"], seed + 200)
        out64 = restatement(sd, cfg, points, centre, nbr, torch.float64).numpy()
        out32 = restatement(sd, cfg, points, centre, nbr, torch.float32).numpy()
        _SWEEP_CACHE[name] = dict(cfg=cfg, sd=sd, points=points, centre_idx=centre, nbr_idx=nbr, out64=out64,
                                  e32=float(np.abs(out32.astype(np.float64) - out64).max()))
    return _SWEEP_CACHE[name]
