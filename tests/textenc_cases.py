"""The text tower's edge cases: configurations, prompts and float64 references shared by tests/test_textenc_edges_cpu.py (which pins
the references and asserts what every case is said to reach) and tests/test_textenc_edges_gpu.py (which runs libtamf_textenc.so on
them).  Built on tests/textenc_restatement.py: seeded weights, seeded or hand-written ids, `forward` in float64 and e32 =
`float32_error`, the unit of the project's 4 * e32 gate.  Everything is computed at test time and cached per process; nothing here is
stored.

case            V, ctx, W, heads, layers, E        what it reaches
ctx2            3, 2, 64, 1, 1, 16                 the smallest context
vocab2          2, 2, 64, 1, 1, 16                 the smallest vocabulary: all four rows over {0, 1}
vocab2_ctx16    2, 16, 64, 1, 1, 16                the same vocabulary, hand-written rows whose first 1 sits at 0, 5, 15 or nowhere
w1024           64, 16, 1024, 16, 1, 1024          the widest model and projection: 3072- and 4096-column GEMMs, K = 4096 in c_proj
w192            97, 40, 192, 3, 2, 80              an odd head count, 9 column tiles of the QKV GEMM, a 64 + 16 column projection
ctx128_edges    300, 128, 128, 2, 2, 48            prompt lengths 16k - 1, 16k, 16k + 1 for every k: every query-block, round and Lp edge
                                                   of attn_kernel (M = 1599 packed rows)
deep            64, 16, 64, 1, 24, 32              24 layers: 48 in-place rewrites of the residual stream
sharp           64, 48, 128, 2, 2, 32              q and k rows of every in_proj_weight times 8: scores beyond the float32 exp range
rows_63/64/65   tiny                               packed row counts on either side of the GEMM's 64-row tile
tail_64/65      tiny                               64 and 65 prompts: the tail LayerNorm and projection across a row tile"""
from __future__ import annotations

from typing import Dict

import numpy as np

import textenc_restatement as R

TINY = R.CONFIGS["tiny"]
SWEEP_CFG = {
    "ctx2": dict(vocab_size=3, context_length=2, width=64, num_heads=1, num_layers=1, embed_dim=16),
    "vocab2": dict(vocab_size=2, context_length=2, width=64, num_heads=1, num_layers=1, embed_dim=16),
    "vocab2_ctx16": dict(vocab_size=2, context_length=16, width=64, num_heads=1, num_layers=1, embed_dim=16),
    "w1024": dict(vocab_size=64, context_length=16, width=1024, num_heads=16, num_layers=1, embed_dim=1024),
    "w192": dict(vocab_size=97, context_length=40, width=192, num_heads=3, num_layers=2, embed_dim=80),
    "ctx128_edges": dict(vocab_size=300, context_length=128, width=128, num_heads=2, num_layers=2, embed_dim=48),
    "deep": dict(vocab_size=64, context_length=16, width=64, num_heads=1, num_layers=24, embed_dim=32),
    "sharp": dict(vocab_size=64, context_length=48, width=128, num_heads=2, num_layers=2, embed_dim=32),
    "rows_63": TINY, "rows_64": TINY, "rows_65": TINY, "tail_64": TINY, "tail_65": TINY,
}
# EOT positions in batch order (the prompt has L = e + 1 rows); None: the ids are written by hand in `_ids`
EOT = {
    "ctx2": [0, 1],
    "vocab2": None,
    "vocab2_ctx16": None,
    "w1024": [15, 0, 7, 12, 3, 15],
    "w192": [39, 0, 16, 31, 32, 33, 7],
    "ctx128_edges": [e for k in range(1, 9) for e in (16 * k - 2, 16 * k - 1, 16 * k) if e < 128],
    "deep": [15, 0, 1, 9],
    "sharp": [47, 0, 16, 31, 5],
    "rows_63": [15, 15, 15, 14],  # the tile's last row has no packed row
    "rows_64": [15, 15, 15, 15],  # exactly one tile
    "rows_65": [15, 15, 15, 15, 0],  # a second tile with one live row
    "tail_64": [(7 * i) % 16 for i in range(64)],
    "tail_65": [(7 * i) % 16 for i in range(65)],
}
SWEEP = tuple(SWEEP_CFG)
WEIGHT_SEED = {n: 520 + i for i, n in enumerate(SWEEP)}
IDS_SEED = {n: 620 + i for i, n in enumerate(SWEEP)}
TINY_WEIGHTS = ("rows_63", "rows_64", "rows_65", "tail_64", "tail_65")  # these run on R.case("tiny")'s weights
SHARP_SCALE = 8.0
EXP_OVERFLOW = 88.7  # float32 exp overflows above 88.72


def sharpen(sd, cfg, scale):
    """the q and k rows (the first 2W) of every attn.in_proj_weight times `scale`, rounded back to fp16-representable values: scores
    grow by scale^2 (up to the biases), the value path and so the outputs' magnitude stay"""
    W = int(cfg["width"])
    out = dict(sd)
    for k, v in sd.items():
        if k.endswith("attn.in_proj_weight"):
            w = v.copy()
            w[:2 * W] *= np.float32(scale)
            out[k] = w.astype(np.float16).astype(np.float32)
            assert np.isfinite(out[k]).all()
    return out


def _ids(name, cfg):
    if name == "vocab2":
        return np.array([[0, 0], [0, 1], [1, 0], [1, 1]], dtype=np.int32)
    if name == "vocab2_ctx16":  # the EOT position is the first 1; an all-zero row reads position 0
        ids = np.zeros((5, 16), dtype=np.int32)
        ids[0, 0] = 1
        ids[1, 5:] = 1
        ids[2, 15] = 1
        ids[4, [9, 12]] = 1
        return ids
    return R.seeded_ids(cfg, EOT[name], IDS_SEED[name])


def _weights(name, cfg):
    if name in TINY_WEIGHTS:
        return R.case("tiny")["sd"]
    sd = R.seeded_state_dict(cfg, WEIGHT_SEED[name])
    return sharpen(sd, cfg, SHARP_SCALE) if name == "sharp" else sd


def _reference(cfg, sd, ids):
    out64 = R.forward(sd, cfg, ids)
    return dict(cfg=cfg, sd=sd, ids=ids, eot=np.argmax(ids, axis=1), out64=out64, e32=R.float32_error(sd, cfg, ids, out64))


_CACHE: Dict[str, dict] = {}


def sweep_case(name: str) -> dict:
    """cfg, sd, ids (B, ctx) int32, eot (B,), out64 (the float64 restatement) and e32 (the CPU float32 torch.nn assembly's error
    against it, relative to max |out64|) of one SWEEP case: computed once and shared, do not modify"""
    if name not in _CACHE:
        cfg = SWEEP_CFG[name]
        _CACHE[name] = _reference(cfg, _weights(name, cfg), _ids(name, cfg))
    return _CACHE[name]


def packed_rows(name: str) -> int:
    return int((sweep_case(name)["eot"] + 1).sum())


# ---- batches beyond one call of the wrapper (MAX_PROMPTS_PER_CALL = 256): tiny's weights, EOT positions (7 i) % 16 ----
CHUNK_SIZES = (257, 513)


def chunk_case(B: int) -> dict:
    key = f"chunk_{B}"
    if key not in _CACHE:
        _CACHE[key] = _reference(TINY, R.case("tiny")["sd"], R.seeded_ids(TINY, [(7 * i) % 16 for i in range(B)], 700 + B))
    return _CACHE[key]


# ---- the library's largest batch in one call ----
BIG_B = 65535  # the library's limit: attn_kernel's grid y
BIG_CFG = dict(vocab_size=8, context_length=16, width=64, num_heads=1, num_layers=1, embed_dim=16)
BIG_LONG = {0: 15, 32767: 9, 65534: 4}  # batch position -> EOT position of the few longer prompts


def big_case() -> dict:
    """cfg, sd, ids (65535, 16), `distinct` (11, 16) ids - the prompts [v, 0, ...] for v = 0 .. 7, then the three long ones - and
    `which` (65535,): the row of `distinct` whose encoding every batch row must equal bit for bit.  A short prompt's EOT position is 0:
    its first id is i % 8 and no later id is larger, so nothing behind the first id reaches the result."""
    if "big" not in _CACHE:
        V, C = BIG_CFG["vocab_size"], BIG_CFG["context_length"]
        rng = np.random.default_rng(811)
        first = (np.arange(BIG_B) % V).astype(np.int32)
        ids = np.minimum(rng.integers(0, V, (BIG_B, C), dtype=np.int32), first[:, None])
        ids[:, 0] = first
        which = first.astype(np.int64)
        long_ids = R.seeded_ids(BIG_CFG, list(BIG_LONG.values()), 812)
        distinct = np.zeros((V + len(BIG_LONG), C), dtype=np.int32)
        distinct[:V, 0] = np.arange(V)
        for j, pos in enumerate(BIG_LONG):
            ids[pos], distinct[V + j], which[pos] = long_ids[j], long_ids[j], V + j
        _CACHE["big"] = dict(cfg=BIG_CFG, sd=R.seeded_state_dict(BIG_CFG, 810), ids=ids, distinct=distinct, which=which)
    return _CACHE["big"]


# ---- the M * 4 * width < 2^31 line ----
LINE_CFG = dict(vocab_size=4, context_length=128, width=1024, num_heads=16, num_layers=1, embed_dim=16)
LINE_B = 4096  # 4096 prompts of 128 rows: M * 4 * 1024 == 2^31


def line_ids(short_one: bool) -> np.ndarray:
    """(4096, 128) ids with every EOT at 127 (M = 524288); `short_one`: the last prompt's EOT at 126 (M = 524287)"""
    ids = np.ones((LINE_B, LINE_CFG["context_length"]), dtype=np.int32)
    ids[:, 127] = 3
    if short_one:
        ids[-1, 126], ids[-1, 127] = 3, 0
    return ids
