"""The text tower of CLIP restated twice, and the seeded inputs of its tests.

`forward`        float64 numpy, written from the published model definition (Radford et al. 2021, the text side): the full context
                 with an explicit additive mask and plain matmuls - no packing, no early exit at the EOT row.
`TorchTower`     the same model assembled from torch.nn.Embedding / MultiheadAttention / LayerNorm / Linear, whose parameter names
                 are the archive's key names (they are torch's own), in any dtype: the second, independent implementation that pins
                 the definition, and in float32 the unit of the GPU gate.
`seeded_state_dict`  deterministic "trained-like" weights: LayerNorm gains near 1 with small offsets, linear weights of std
                 fan_in^-0.5 with small biases, embeddings of std 0.02 / 0.01 - outputs of order 1 to 10.  With fp16=True (default)
                 the tensors the reference keeps in fp16 are fp16-representable, as in OpenAI's archive.
Weights are regenerated at test time and never stored (the full model has 63 M parameters with its token table);
tools/capture_textenc_golden.py records their checksum beside the outputs."""
from __future__ import annotations

import hashlib
from collections import OrderedDict
from typing import Dict, Mapping, Optional

import numpy as np

CONFIGS = {
    "tiny": dict(vocab_size=64, context_length=16, width=64, num_heads=1, num_layers=2, embed_dim=32),
    "mid": dict(vocab_size=512, context_length=24, width=128, num_heads=2, num_layers=3, embed_dim=48),
    "full": dict(vocab_size=49408, context_length=77, width=512, num_heads=8, num_layers=12, embed_dim=512),  # ViT-B/32
}
WEIGHT_SEED = {"tiny": 301, "mid": 302, "full": 303}
IDS_SEED = {"tiny": 401, "mid": 402, "full": 403}
# EOT positions of the fixture's prompts, in batch order.  They cover 0 (an all-zero id row), 1, 2, 15, 16, 17, 21 and ctx - 1 as far
# as the context has them, and the packed row count sum(e + 1) crosses the GEMM's 64-row tile boundary inside a prompt.
EOT_POSITIONS = {
    "tiny": [15, 0, 1, 2, 7, 15, 9, 15, 3, 15, 11],
    "mid": [21, 0, 1, 2, 15, 16, 17, 23, 5, 21, 23],
    "full": [21, 0, 1, 2, 15, 16, 17, 76, 21, 9, 40],
}
GEMM_TILE = 64


def is_fp16_key(key: str) -> bool:
    """the tensors the reference's convert_weights turns into fp16: Linear and attention parameters, text_projection"""
    return key == "text_projection" or ".attn." in key or ".mlp." in key


def round_fp16(sd: Mapping[str, np.ndarray]) -> Dict[str, np.ndarray]:
    return {k: (v.astype(np.float16).astype(np.float32) if is_fp16_key(k) else v) for k, v in sd.items()}


def seeded_state_dict(cfg: Mapping[str, int], seed: int, fp16: bool = True) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(seed)
    V, C, W, E, L = (int(cfg[k]) for k in ("vocab_size", "context_length", "width", "embed_dim", "num_layers"))
    sd: Dict[str, np.ndarray] = OrderedDict()

    def normal(shape, std):
        return (std * rng.standard_normal(shape, dtype=np.float32)).astype(np.float32)

    def ln(name):
        sd[name + ".weight"] = (1.0 + normal((W,), 0.1)).astype(np.float32)
        sd[name + ".bias"] = normal((W,), 0.05)

    def lin(wname, bname, o, i):
        sd[wname] = normal((o, i), i ** -0.5)
        sd[bname] = normal((o,), 0.02)

    sd["token_embedding.weight"] = normal((V, W), 0.02)
    sd["positional_embedding"] = normal((C, W), 0.01)
    for l in range(L):
        p = f"transformer.resblocks.{l}."
        ln(p + "ln_1")
        lin(p + "attn.in_proj_weight", p + "attn.in_proj_bias", 3 * W, W)
        lin(p + "attn.out_proj.weight", p + "attn.out_proj.bias", W, W)
        ln(p + "ln_2")
        lin(p + "mlp.c_fc.weight", p + "mlp.c_fc.bias", 4 * W, W)
        lin(p + "mlp.c_proj.weight", p + "mlp.c_proj.bias", W, 4 * W)
    ln("ln_final")
    sd["text_projection"] = normal((W, E), W ** -0.5)
    return round_fp16(sd) if fp16 else dict(sd)


def state_checksum(sd: Mapping[str, np.ndarray]) -> str:
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k], dtype=np.float32).tobytes())
    return h.hexdigest()


def seeded_ids(cfg: Mapping[str, int], eot_positions, seed: int) -> np.ndarray:
    """(B, ctx) int32: row b holds ids drawn from [1, V - 1) before position e_b, the EOT id V - 1 at e_b and zeros behind it, as the
    reference pads; e_b = 0 gives an all-zero row (its first argmax is position 0)"""
    rng = np.random.default_rng(seed)
    V, C = int(cfg["vocab_size"]), int(cfg["context_length"])
    ids = np.zeros((len(eot_positions), C), dtype=np.int32)
    for b, e in enumerate(eot_positions):
        assert 0 <= e < C
        if e > 0:
            ids[b, :e] = rng.integers(1, V - 1, e)
            ids[b, e] = V - 1
    assert np.array_equal(np.argmax(ids, axis=1), np.asarray(eot_positions))
    return ids


def _layer_norm(x, g, b):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-5) * g + b


def forward(sd: Mapping[str, np.ndarray], cfg: Mapping[str, int], ids, length: Optional[int] = None) -> np.ndarray:
    """(B, ctx) ids -> (B, embed_dim) float64.  `length`: evaluate the first `length` positions only (every row's EOT position must
    lie inside; the causal mask says the result is the same)"""
    ids = np.asarray(ids)
    W, H = int(cfg["width"]), int(cfg["num_heads"])
    eot = np.argmax(ids, axis=1)  # the first index among equals
    T = ids.shape[1] if length is None else int(length)
    assert eot.max() < T
    t = lambda k: np.asarray(sd[k]).astype(np.float64)  # noqa: E731
    x = t("token_embedding.weight")[ids[:, :T]] + t("positional_embedding")[:T]
    B = x.shape[0]
    mask = np.triu(np.full((T, T), -np.inf), 1)
    for l in range(int(cfg["num_layers"])):
        p = f"transformer.resblocks.{l}."
        qkv = _layer_norm(x, t(p + "ln_1.weight"), t(p + "ln_1.bias")) @ t(p + "attn.in_proj_weight").T + t(p + "attn.in_proj_bias")
        q, k, v = (a.reshape(B, T, H, W // H).transpose(0, 2, 1, 3) for a in np.split(qkv, 3, axis=-1))
        s = q @ k.transpose(0, 1, 3, 2) * (W // H) ** -0.5 + mask
        s = np.exp(s - s.max(-1, keepdims=True))
        a = (s / s.sum(-1, keepdims=True)) @ v
        x = x + a.transpose(0, 2, 1, 3).reshape(B, T, W) @ t(p + "attn.out_proj.weight").T + t(p + "attn.out_proj.bias")
        h = _layer_norm(x, t(p + "ln_2.weight"), t(p + "ln_2.bias")) @ t(p + "mlp.c_fc.weight").T + t(p + "mlp.c_fc.bias")
        h = h / (1.0 + np.exp(-1.702 * h))  # QuickGELU
        x = x + h @ t(p + "mlp.c_proj.weight").T + t(p + "mlp.c_proj.bias")
    x = _layer_norm(x, t("ln_final.weight"), t("ln_final.bias"))
    return x[np.arange(B), eot] @ t("text_projection")


def layer0_scores(sd: Mapping[str, np.ndarray], cfg: Mapping[str, int], ids) -> np.ndarray:
    """(B, H, ctx, ctx) float64: the scaled scores q . k^T * 64^-0.5 of the first block BEFORE the mask (entry [b, h, i, j]: query i
    against key j), the same lines as `forward`'s first iteration"""
    ids = np.asarray(ids)
    W, H = int(cfg["width"]), int(cfg["num_heads"])
    t = lambda k: np.asarray(sd[k]).astype(np.float64)  # noqa: E731
    x = t("token_embedding.weight")[ids] + t("positional_embedding")[:ids.shape[1]]
    B, T = ids.shape
    p = "transformer.resblocks.0."
    qkv = _layer_norm(x, t(p + "ln_1.weight"), t(p + "ln_1.bias")) @ t(p + "attn.in_proj_weight").T + t(p + "attn.in_proj_bias")
    q, k, _ = (a.reshape(B, T, H, W // H).transpose(0, 2, 1, 3) for a in np.split(qkv, 3, axis=-1))
    return q @ k.transpose(0, 1, 3, 2) * (W // H) ** -0.5


def torch_tower(sd: Mapping[str, np.ndarray], cfg: Mapping[str, int], dtype, device="cpu"):
    """the model as torch.nn modules with the state dict loaded strictly: callable (B, ctx) ids -> (B, embed_dim) tensor"""
    import torch
    from torch import nn

    W, H = int(cfg["width"]), int(cfg["num_heads"])

    class QuickGELU(nn.Module):
        def forward(self, x):
            return x * torch.sigmoid(1.702 * x)

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.ln_1 = nn.LayerNorm(W, eps=1e-5)
            self.attn = nn.MultiheadAttention(W, H, batch_first=True)
            self.ln_2 = nn.LayerNorm(W, eps=1e-5)
            self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(W, 4 * W)), ("gelu", QuickGELU()), ("c_proj", nn.Linear(4 * W, W))]))

        def forward(self, x, mask):
            y = self.ln_1(x)
            x = x + self.attn(y, y, y, need_weights=False, attn_mask=mask)[0]
            return x + self.mlp(self.ln_2(x))

    class Transformer(nn.Module):
        def __init__(self):
            super().__init__()
            self.resblocks = nn.ModuleList([Block() for _ in range(int(cfg["num_layers"]))])

    class Tower(nn.Module):
        def __init__(self):
            super().__init__()
            self.token_embedding = nn.Embedding(int(cfg["vocab_size"]), W)
            self.positional_embedding = nn.Parameter(torch.empty(int(cfg["context_length"]), W))
            self.transformer = Transformer()
            self.ln_final = nn.LayerNorm(W, eps=1e-5)
            self.text_projection = nn.Parameter(torch.empty(W, int(cfg["embed_dim"])))

        def forward(self, ids):
            ids = torch.as_tensor(np.asarray(ids)).long().to(self.positional_embedding.device)
            T = ids.shape[1]
            x = self.token_embedding(ids) + self.positional_embedding[:T]
            mask = torch.full((T, T), float("-inf"), dtype=x.dtype, device=x.device).triu_(1)
            for blk in self.transformer.resblocks:
                x = blk(x, mask)
            x = self.ln_final(x)
            return x[torch.arange(ids.shape[0], device=x.device), ids.argmax(dim=-1)] @ self.text_projection

    m = Tower()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(device=device, dtype=dtype)
    m.train()  # (no dropout anywhere; training mode keeps MultiheadAttention on its plain, unfused path)
    for prm in m.parameters():
        prm.requires_grad_(False)
    return m


def float32_error(sd, cfg, ids, out64) -> float:
    """max |float32 torch.nn assembly on the CPU - float64 restatement| / max |restatement|: the unit of the GPU gate"""
    import torch

    with torch.no_grad():
        out32 = torch_tower(sd, cfg, torch.float32)(ids).numpy().astype(np.float64)
    return float(np.abs(out32 - out64).max() / np.abs(out64).max())


_CASE_CACHE: Dict[str, dict] = {}


def case(name: str) -> dict:
    """cfg, seeded weights and ids of one configuration, computed once and shared (do not modify)"""
    if name not in _CASE_CACHE:
        cfg = CONFIGS[name]
        _CASE_CACHE[name] = dict(cfg=cfg, sd=seeded_state_dict(cfg, WEIGHT_SEED[name]), ids=seeded_ids(cfg, EOT_POSITIONS[name], IDS_SEED[name]))
    return _CASE_CACHE[name]
