"""CPU: the references of tests/test_textenc_edges_gpu.py.  For every case of tests/textenc_cases.py: the float64 numpy restatement
agrees with the float64 torch.nn assembly (the gate of tests/test_textenc_cpu.py: e32 / 1000 relative to max |out|), e32 lies in
(0, 1e-5), and what the case is said to reach is asserted from its data - so a case that no longer reaches its edge fails here, on
any machine.  And the host-only part of the C interface around the library's two size limits."""
import ctypes
import os
import sys
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import textenc_cases as C  # noqa: E402
import textenc_restatement as R  # noqa: E402


def _pinned(tag, c):
    with torch.no_grad():
        got = R.torch_tower(c["sd"], c["cfg"], torch.float64)(c["ids"]).numpy()
    out64, e32 = c["out64"], c["e32"]
    err = float(np.abs(got - out64).max() / np.abs(out64).max())
    print(f"{tag}: torch.nn float64 against the restatement {err:.3e}, e32 = {e32:.3e}, max|out| = {np.abs(out64).max():.2f}")
    assert out64.dtype == np.float64 and out64.shape == (c["ids"].shape[0], c["cfg"]["embed_dim"]) and np.isfinite(out64).all()
    assert c["ids"].dtype == np.int32 and c["ids"].min() >= 0 and c["ids"].max() < c["cfg"]["vocab_size"]
    assert 0 < e32 < 1e-5
    assert err <= e32 / 1000


@pytest.mark.parametrize("name", C.SWEEP)
def test_the_sweep_references_are_pinned(name):
    c = C.sweep_case(name)
    _pinned(name, c)
    if C.EOT[name] is not None:
        assert c["eot"].tolist() == C.EOT[name]
    for k, v in c["sd"].items():  # fp16-representable where the reference keeps fp16
        assert v.dtype == np.float32 and (not R.is_fp16_key(k) or np.array_equal(v.astype(np.float16).astype(np.float32), v)), k


@pytest.mark.parametrize("B", C.CHUNK_SIZES)
def test_the_chunk_references_are_pinned(B):
    c = C.chunk_case(B)
    _pinned(f"chunk {B}", c)
    assert c["ids"].shape == (B, 16) and c["eot"].tolist() == [(7 * i) % 16 for i in range(B)]
    assert B % 256 == 1 and R.state_checksum(c["sd"]) == R.state_checksum(R.case("tiny")["sd"])


def test_the_cases_sit_at_the_ends_of_the_accepted_ranges():
    """against the ranges of include/tamf_textenc.h (tamf_textenc_model_create refuses anything outside them)"""
    cfg = C.SWEEP_CFG
    assert cfg["ctx2"]["context_length"] == 2 and C.sweep_case("ctx2")["eot"].tolist() == [0, 1]
    assert cfg["vocab2"]["vocab_size"] == 2 and cfg["vocab2"]["context_length"] == 2
    assert sorted(map(tuple, C.sweep_case("vocab2")["ids"].tolist())) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert C.sweep_case("vocab2")["eot"].tolist() == [0, 1, 0, 0]
    v16 = C.sweep_case("vocab2_ctx16")
    assert cfg["vocab2_ctx16"]["vocab_size"] == 2 and v16["eot"].tolist() == [0, 5, 15, 0, 9] and not v16["ids"][3].any()
    assert v16["ids"][1, 6:].all() and v16["ids"][4, 12] == 1  # the first of several equal ids counts
    w = cfg["w1024"]
    assert (w["width"], w["num_heads"], w["embed_dim"]) == (1024, 16, 1024) and 4 * w["width"] == 4096
    o = cfg["w192"]
    assert o["num_heads"] == 3 and 3 * o["width"] // R.GEMM_TILE == 9 and o["embed_dim"] % 64 == 16 and o["embed_dim"] > 64
    assert {31, 32, 33, 39, 0} <= set(C.EOT["w192"]) and o["context_length"] == 40
    assert cfg["deep"]["num_layers"] == 24
    for n in C.SWEEP:
        assert cfg[n]["num_heads"] * 64 == cfg[n]["width"] and cfg[n]["embed_dim"] % 16 == 0


def test_ctx128_edges_has_every_block_round_and_panel_edge():
    """attn_kernel: a wave takes 16 queries, a round 4 waves, the panels are sized by Lp = round_up(longest prompt, 16): every
    L = 16k - 1, 16k, 16k + 1 up to the context's 128"""
    c = C.sweep_case("ctx128_edges")
    L = set((c["eot"] + 1).tolist())
    want = {15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127, 128}
    assert L == want and len(c["eot"]) == len(want)
    assert {16 * k + d for k in range(1, 8) for d in (-1, 0, 1)} | {127, 128} == L
    assert C.packed_rows("ctx128_edges") == 1599
    assert c["cfg"]["context_length"] == 128 and c["cfg"]["num_heads"] == 2


def test_sharp_scores_leave_the_float32_exp_range():
    """what makes `sharp` a test of the softmax: among the scores attn_kernel computes in layer 0 (float64 here) an unmasked one lies
    beyond +-100 - exp without the row maximum subtracted overflows at 88.7 - and a masked column that sits in its query's score
    panel (query i's block sees keys up to 16 (i / 16 + 1), the prompt has L of them) holds more than the row's unmasked maximum by
    over 104, the float32 exp's underflow to zero: a maximum taken over the panel would zero the whole row"""
    c = C.sweep_case("sharp")
    s = R.layer0_scores(c["sd"], c["cfg"], c["ids"])
    assert s.shape == (5, 2, 48, 48)
    top, margin = 0.0, -np.inf
    for b, e in enumerate(c["eot"]):
        L = int(e) + 1
        for i in range(L):
            seen = s[b, :, i, :i + 1]
            top = max(top, float(np.abs(seen).max()))
            kend = min(16 * (i // 16 + 1), L)
            if kend > i + 1:
                margin = max(margin, float((s[b, :, i, i + 1:kend].max(-1) - seen.max(-1)).max()))
    print(f"sharp: max |unmasked score| = {top:.1f}, largest masked-over-unmasked margin inside a panel = {margin:.1f}")
    assert top > 100 > C.EXP_OVERFLOW
    assert margin > 0
    assert margin > 104
    # the same weights without the factor stay far inside the range: the factor is what the case is
    mild = R.layer0_scores(R.seeded_state_dict(c["cfg"], C.WEIGHT_SEED["sharp"]), c["cfg"], c["ids"])
    assert np.abs(mild).max() < 10 and C.SHARP_SCALE == 8.0
    assert 1.0 < np.abs(c["out64"]).max() < 10.0


def test_packed_row_counts_around_the_gemm_tile():
    assert [C.packed_rows(n) for n in ("rows_63", "rows_64", "rows_65")] == [63, 64, 65] and R.GEMM_TILE == 64
    assert C.sweep_case("tail_64")["ids"].shape[0] == 64 and C.sweep_case("tail_65")["ids"].shape[0] == 65
    for n in C.TINY_WEIGHTS:
        assert C.SWEEP_CFG[n] == R.CONFIGS["tiny"] and C.sweep_case(n)["sd"] is R.case("tiny")["sd"]


def test_the_largest_batch_is_made_of_eleven_distinct_prompts():
    c = C.big_case()
    ids, distinct, which = c["ids"], c["distinct"], c["which"]
    assert ids.shape == (65535, 16) and ids.dtype == np.int32 and distinct.shape == (11, 16)
    eot = np.argmax(ids, axis=1)
    assert {p: int(eot[p]) for p in C.BIG_LONG} == C.BIG_LONG and (np.delete(eot, list(C.BIG_LONG)) == 0).all()
    assert np.array_equal(ids[:, 0][eot == 0] % 8, (np.arange(65535) % 8)[eot == 0]) and ids.max() == 7
    # up to its EOT position every prompt is its row of `distinct`; behind it the short ones differ (ids that reach no result)
    d_eot = np.argmax(distinct, axis=1)
    assert np.array_equal(d_eot[which], eot)
    keep = np.arange(16)[None] <= eot[:, None]
    assert np.array_equal(np.where(keep, ids, 0), np.where(keep, distinct[which], 0))
    assert (ids[eot == 0][:, 1:] != 0).any() and len(np.unique(which)) == 11


def _model(lib, T, cfg):
    m = c_void_p()
    assert lib.tamf_textenc_model_create(ctypes.byref(T._Config(**cfg)), ctypes.byref(m)) == 0
    return m


def test_workspace_bytes_at_the_batch_limit_and_the_2_31_line():
    """host only (a model that was never finalised answers): 65535 prompts is the limit, and total_rows * 4 * width must stay
    below 2^31"""
    from oakink2_tamf_amd.model import text_encoder as T

    lib = T._bind()
    m = _model(lib, T, R.CONFIGS["tiny"])
    assert lib.tamf_textenc_workspace_bytes(m, 65536, 65536) == 0
    assert lib.tamf_textenc_workspace_bytes(m, 65535, 65535) > 0 and lib.tamf_textenc_workspace_bytes(m, 65535, 65535 * 16) > 0
    assert lib.tamf_textenc_destroy(m) == 0
    m = _model(lib, T, C.LINE_CFG)
    W, B = C.LINE_CFG["width"], C.LINE_B
    line = 2 ** 31 // (4 * W)
    assert line * 4 * W == 2 ** 31 and line == B * C.LINE_CFG["context_length"]
    assert lib.tamf_textenc_workspace_bytes(m, B, line) == 0
    assert lib.tamf_textenc_workspace_bytes(m, B + 1, line + 1) == 0
    below = int(lib.tamf_textenc_workspace_bytes(m, B, line - 1))
    assert below >= 4 * (line - 1) * 10 * W and below % 16 == 0  # x, y, qkv (3), ao, hh (4): ten W-wide float32 rows per packed row
    assert lib.tamf_textenc_destroy(m) == 0
    for short_one, M in ((False, line), (True, line - 1)):
        ids = C.line_ids(short_one)
        assert ids.shape == (B, 128) and int((np.argmax(ids, axis=1) + 1).sum()) == M and ids.max() < C.LINE_CFG["vocab_size"]
