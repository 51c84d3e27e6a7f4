"""GPU: the native text tower (libtamf_textenc.so through model/text_encoder.py, and its C interface directly) across the ranges
tamf_textenc_model_create accepts and at the edges of its kernels and of the wrapper's call chunking - not only at the three
configurations of tests/test_textenc_gpu.py.  Cases and float64 references: tests/textenc_cases.py, pinned without a GPU by
tests/test_textenc_edges_cpu.py.

Tolerance: the project's rule, unchanged (tests/test_textenc_gpu.py): e32 = the CPU float32 torch.nn assembly's error against the
float64 restatement on the case's own inputs, relative to max |out64|; the gate on the HIP output is 4 * e32.  Everything else is
compared bit for bit: the header promises that a prompt's output bits depend on its ids up to the EOT position and on the model only.

What is reached (attn_kernel: 16 queries per wave, 4 waves per round, panels sized by Lp = round_up(longest prompt of the call, 16)):
  sweep parity      every case of textenc_cases.SWEEP: context 2, vocabulary 2, width 1024 / embed_dim 1024, three heads with an
                    80-column projection, 24 layers, every prompt length 16k - 1, 16k, 16k + 1 up to 128, scores beyond +-100,
                    63 / 64 / 65 packed rows, 64 / 65 prompts
  alone = batch     ctx128_edges, sharp, w192: a prompt alone runs with panels of its own Lp, in the batch with the longest's
  chunked calls     257 and 513 prompts through the wrapper's calls of 256; four back-to-back calls of 1, 300, 1 and 40 prompts on
                    one encoder (the pinned row-map staging buffer reused, grown and reused again), on the default and on a side stream
  C interface       out_dev and an exactly sized workspace inside sentinel-filled tensors, every refusal of tamf_textenc_encode,
                    65535 prompts in one call, and both sides of the M * 4 * width < 2^31 line
The back-to-back test cannot fail deterministically for a missing wait on the staging buffer's event (the host would have to
overwrite the buffer before the copy engine has read it); it runs the sequence once and checks the bits.

Measured on an MI355X, first run (relative to max |out64|; gate: ratio <= 4).  e32 is computed by the CPU of the machine that runs the
test, so it moves with that CPU's BLAS: the same cases gave e32 between 0.6 and 1.6 times these values on another CPU.
  case            HIP err     e32         ratio
  ctx2            4.409e-07   4.173e-07   1.06
  vocab2          5.465e-07   4.884e-07   1.12
  vocab2_ctx16    3.209e-07   3.236e-07   0.99
  w1024           1.370e-06   8.448e-07   1.62
  w192            8.046e-07   6.069e-07   1.33
  ctx128_edges    8.706e-07   6.127e-07   1.42
  deep            5.412e-07   4.522e-07   1.20
  sharp           2.162e-06   8.821e-07   2.45
  rows_63         6.871e-07   7.438e-07   0.92
  rows_64         6.797e-07   5.851e-07   1.16
  rows_65         4.885e-07   3.947e-07   1.24
  tail_64         6.649e-07   5.817e-07   1.14
  tail_65         9.522e-07   5.238e-07   1.82
  tiny x 257      8.373e-07   6.666e-07   1.26
  tiny x 513      6.636e-07   5.560e-07   1.19"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import textenc_cases as C  # noqa: E402
import textenc_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE_FACTOR = 4.0
SENT = -12345.0  # outputs are of order 1 to 10; no activation comes near
INVALID = -1  # TAMF_ERR_INVALID of include/tamf_hip.h (pinned by tests/test_textenc_cpu.py)
_ENC = {}


def _new_encoder(cfg, sd):
    from oakink2_tamf_amd.model.text_encoder import HipClipTextEncoder

    enc = HipClipTextEncoder(cfg, device=DEV)
    enc.load_state_dict(sd)
    return enc


def encoder(name):
    """one encoder per set of weights, shared by the tests (do not load or close it); the cases on tiny's weights share one"""
    key = "tiny" if name == "tiny" or name in C.TINY_WEIGHTS else name
    if key not in _ENC:
        c = R.case("tiny") if key == "tiny" else C.sweep_case(key)
        _ENC[key] = _new_encoder(c["cfg"], c["sd"])
    return _ENC[key]


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _gate(tag, out, c):
    out64, e32 = c["out64"], c["e32"]
    assert out.shape == out64.shape and out.dtype == np.float32 and np.isfinite(out).all()
    err = float(np.abs(out.astype(np.float64) - out64).max() / np.abs(out64).max())
    print(f"textenc edges {tag}: HIP {err:.3e}, CPU float32 e32 {e32:.3e}, ratio {err / e32:.2f} (gate {GATE_FACTOR:.0f})")
    assert 0 < e32 < 1e-5
    assert err <= GATE_FACTOR * e32


# ---- the accepted configurations and the packed-row edges ----
@pytest.mark.parametrize("name", C.SWEEP)
def test_sweep_parity_with_the_float64_restatement(name):
    c = C.sweep_case(name)
    out = encoder(name).encode_tokens(c["ids"])
    assert out.dtype == torch.float32 and tuple(out.shape) == (c["ids"].shape[0], c["cfg"]["embed_dim"])
    _gate(name, out.cpu().numpy(), c)


# ---- attention edges, bit for bit ----
@pytest.mark.parametrize("name", ["ctx128_edges", "sharp", "w192"])
def test_every_prompt_alone_gives_its_bits_in_the_batch(name):
    """alone, a prompt's K / V / score panels are sized by its own Lp and its query blocks fill other rounds' waves than beside a
    longer prompt; the bits are the same"""
    c, enc = C.sweep_case(name), encoder(name)
    ids = c["ids"]
    batch = enc.encode_tokens(ids).cpu().numpy()
    assert np.isfinite(batch).all()
    for b in range(ids.shape[0]):
        assert np.array_equal(bits(enc.encode_tokens(ids[b: b + 1]))[0], batch[b].view(np.uint32)), (b, int(c["eot"][b]))
    assert np.array_equal(bits(enc.encode_tokens(ids[::-1].copy()))[::-1], batch.view(np.uint32))


@pytest.mark.parametrize("name", ["ctx128_edges", "sharp", "w192"])
def test_ids_behind_the_eot_position_change_no_bit(name):
    c, enc = C.sweep_case(name), encoder(name)
    ids = c["ids"]
    rng = np.random.default_rng(19)
    other = ids.copy()
    for b, e in enumerate(c["eot"]):  # arbitrary valid ids up to the row's own maximum (the first one counts)
        other[b, e + 1:] = rng.integers(0, int(ids[b, e]) + 1, ids.shape[1] - e - 1)
    assert (other != ids).sum() > ids.shape[1] and np.array_equal(np.argmax(other, axis=1), c["eot"])
    assert np.array_equal(bits(enc.encode_tokens(other)), bits(enc.encode_tokens(ids)))


# ---- the wrapper's calls of 256 prompts ----
@pytest.mark.parametrize("B", C.CHUNK_SIZES)
def test_a_batch_beyond_one_call_is_cut_at_256(B):
    from oakink2_tamf_amd.model.text_encoder import MAX_PROMPTS_PER_CALL

    assert MAX_PROMPTS_PER_CALL == 256
    c, enc = C.chunk_case(B), encoder("tiny")
    ids = c["ids"]
    out = enc.encode_tokens(ids)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, C.TINY["embed_dim"])
    _gate(f"tiny x {B}", out.cpu().numpy(), c)
    got = bits(out)
    for pos in (0, 255, 256, 511, 512):  # the last of a call, the first of the next, the call of one
        if pos < B:
            assert np.array_equal(bits(enc.encode_tokens(ids[pos: pos + 1]))[0], got[pos]), pos
    assert np.array_equal(bits(enc.encode_tokens(ids[256:])), got[256:])
    assert np.array_equal(bits(enc.encode_tokens(ids[:256])), got[:256])
    if B > 260:  # a call of one whose prompt is not the all-zero row that positions 0, 256 and 512 hold ((7 i) % 16 == 0)
        assert ids[259].any() and np.array_equal(bits(enc.encode_tokens(ids[3:260])), got[3:260])


def test_back_to_back_calls_share_the_staging_buffer():
    """1, 300 (calls of 256 and 44), 1 and 40 prompts on one encoder with nothing between the calls: the pinned row map is
    reused, grown twice, and reused by smaller maps while the earlier uploads may still be queued.  Once on the default stream, once
    on a side stream; the expected bits come from a fresh encoder on the default stream, one synchronised call at a time."""
    sd, ids = R.case("tiny")["sd"], C.chunk_case(513)["ids"]
    seq = [ids[5:6], ids[:300], ids[300:301], ids[100:140]]
    fresh = _new_encoder(C.TINY, sd)
    want = []
    for a in seq:
        want.append(bits(fresh.encode_tokens(a)))
        torch.cuda.synchronize()
    fresh.close()
    enc = _new_encoder(C.TINY, sd)
    outs = [enc.encode_tokens(a) for a in seq]
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        assert np.array_equal(bits(o), w), o.shape
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        outs = [enc.encode_tokens(a) for a in seq]
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        assert np.array_equal(bits(o), w), o.shape
    enc.close()


# ---- the C interface directly ----
def _stream():
    return int(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _carve(n, pre, tail):
    """(whole, region): `region` = n floats inside a larger sentinel-filled tensor, `pre` floats from its start"""
    whole = torch.full((pre + n + tail,), SENT, dtype=torch.float32, device=DEV)
    return whole, whole[pre:pre + n]


def _untouched(whole, n, pre):
    return bool((whole[:pre] == SENT).all()) and bool((whole[pre + n:] == SENT).all())


def _raw_encode(enc, tokens, B, out, ws, nbytes):
    """tamf_textenc_encode, then a synchronise -> (status, message).  tokens: an int32 array or None; out / ws: a tensor, an
    address or None"""
    lib = enc._lib
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())  # noqa: E731
    rc = lib.tamf_textenc_encode(enc._model, None if tokens is None else tokens.ctypes.data, B, ptr(out), ptr(ws), nbytes, _stream())
    torch.cuda.synchronize()
    return rc, lib.tamf_textenc_last_error().decode()


def _case_of(name):
    return R.case("tiny") if name == "tiny" else C.sweep_case(name)


@pytest.mark.parametrize("name", ["tiny", "w192"])
def test_c_calls_stay_inside_their_output_and_the_exact_workspace(name):
    """guard rows before and behind out_dev, a workspace of exactly tamf_textenc_workspace_bytes inside a sentinel-filled tensor;
    then the workspace of B * context_length rows, which is always enough"""
    c, enc = _case_of(name), encoder(name)
    ids = np.ascontiguousarray(c["ids"], dtype=np.int32)
    B, ctx = ids.shape
    E = c["cfg"]["embed_dim"]
    M = int((np.argmax(ids, axis=1) + 1).sum())
    want = enc.encode_tokens(ids)
    for rows in (M, B * ctx):
        nbytes = int(enc._lib.tamf_textenc_workspace_bytes(enc._model, B, rows))
        assert nbytes > 0 and nbytes % 16 == 0
        wsw, ws = _carve(nbytes // 4, 64, 1024)
        ow, out = _carve(B * E, 4 * E, 4 * E)
        assert ws.data_ptr() % 16 == 0
        rc, msg = _raw_encode(enc, ids, B, out, ws, nbytes)
        assert rc == 0, msg
        assert _untouched(wsw, nbytes // 4, 64) and _untouched(ow, B * E, 4 * E) and bool((out != SENT).all())
        assert torch.equal(out.reshape(B, E).view(torch.int32), want.view(torch.int32))
    assert int(enc._lib.tamf_textenc_workspace_bytes(enc._model, B, B * ctx)) > int(enc._lib.tamf_textenc_workspace_bytes(enc._model, B, M))


def test_c_calls_refuse_bad_arguments_and_write_nothing():
    c, enc = R.case("tiny"), encoder("tiny")
    ids = np.ascontiguousarray(c["ids"], dtype=np.int32)
    B, E = ids.shape[0], c["cfg"]["embed_dim"]
    M = int((np.argmax(ids, axis=1) + 1).sum())
    nbytes = int(enc._lib.tamf_textenc_workspace_bytes(enc._model, B, M))
    out = torch.full((B * E,), SENT, dtype=torch.float32, device=DEV)
    ws = torch.full((nbytes // 4 + 4,), SENT, dtype=torch.float32, device=DEV)
    many = np.zeros((65536, ids.shape[1]), dtype=np.int32)

    def refused(*words, **kw):
        a = dict(tokens=ids, B=B, out=out, ws=ws, nbytes=nbytes)
        a.update(kw)
        rc, msg = _raw_encode(enc, **a)
        assert rc == INVALID and msg and all(w in msg for w in words), (rc, msg)

    refused("B = 0", B=0)
    refused("B = 65536", "65535", tokens=many, B=65536)
    for k in ("tokens", "out", "ws"):
        refused("null", **{k: None})
    refused("aligned", ws=ws.data_ptr() + 4)
    refused("workspace of %d bytes, need %d" % (nbytes - 1, nbytes), nbytes=nbytes - 1)
    assert bool((out == SENT).all()) and bool((ws == SENT).all())
    rc, msg = _raw_encode(enc, ids, B, out, ws, nbytes)  # the same arguments without a fault are taken
    assert rc == 0, msg
    assert torch.equal(out.reshape(B, E).view(torch.int32), enc.encode_tokens(ids).view(torch.int32)) and bool((ws[-4:] == SENT).all())


def test_65535_prompts_in_one_call():
    """the library's limit and the hardware limit of attn_kernel's grid y: eleven distinct prompts, the short ones with ids behind
    their EOT position that differ from row to row; every output row carries the bits of its prompt encoded alone"""
    c = C.big_case()
    enc = _new_encoder(c["cfg"], c["sd"])
    table = torch.cat([enc.encode_tokens(c["distinct"][j: j + 1]) for j in range(len(c["distinct"]))])
    assert len({r.tobytes() for r in bits(table)}) == len(c["distinct"])
    ids = np.ascontiguousarray(c["ids"], dtype=np.int32)
    B, E = C.BIG_B, c["cfg"]["embed_dim"]
    M = int((np.argmax(ids, axis=1) + 1).sum())
    nbytes = int(enc._lib.tamf_textenc_workspace_bytes(enc._model, B, M))
    assert 150e6 < nbytes < 200e6
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    ow, out = _carve(B * E, 4 * E, 4 * E)
    rc, msg = _raw_encode(enc, ids, B, out, ws, nbytes)
    assert rc == 0, msg
    assert _untouched(ow, B * E, 4 * E)
    want = table[torch.as_tensor(c["which"], device=DEV)]
    same = (out.reshape(B, E).view(torch.int32) == want.view(torch.int32)).all(dim=1)
    assert bool(same.all()), torch.nonzero(~same)[:8].flatten().tolist()
    del ws
    enc.close()


def test_the_2_31_line_is_refused_on_the_host():
    """width 1024, 4096 prompts of 128 rows: M * 4 * width == 2^31 is refused, one row less gets past that check and is refused for the
    (deliberately small) workspace only; neither has enqueued anything"""
    enc = _new_encoder(C.LINE_CFG, R.seeded_state_dict(C.LINE_CFG, 830))
    E = C.LINE_CFG["embed_dim"]
    out = torch.full((C.LINE_B * E,), SENT, dtype=torch.float32, device=DEV)
    ws = torch.full((1024,), SENT, dtype=torch.float32, device=DEV)
    rc, msg = _raw_encode(enc, C.line_ids(False), C.LINE_B, out, ws, 4096)
    assert rc == INVALID and "split the batch" in msg, (rc, msg)
    rc, msg = _raw_encode(enc, C.line_ids(True), C.LINE_B, out, ws, 4096)
    assert rc == INVALID and "workspace of 4096 bytes" in msg and "split" not in msg, (rc, msg)
    assert bool((out == SENT).all()) and bool((ws == SENT).all())
    # the model itself works: one prompt of 128 rows, alone
    one = enc.encode_tokens(C.line_ids(False)[:1])
    assert tuple(one.shape) == (1, E) and bool(torch.isfinite(one).all())
    enc.close()
