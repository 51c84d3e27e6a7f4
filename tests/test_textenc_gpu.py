"""GPU: libtamf_textenc.so through model/text_encoder.py against the float64 restatement's committed fixtures (seeded weights;
tests/textenc_restatement.py, tools/capture_textenc_golden.py), and the properties its packed-row design promises bit for bit."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG_PARENT, ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import textenc_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
BPE = os.path.join(GOLDEN, "clip_bpe_synthetic.txt")

# The gate of the parity test: GATE_FACTOR times e32, the error of the float32 torch.nn assembly on a CPU against the float64
# restatement, relative to max |out| (measured by tools/capture_textenc_golden.py, stored in the fixture).  The kernels do the same
# float32 arithmetic in another summation order; the factor covers order and tile effects.  Measured (relative to max |out|):
#             e32 (CPU float32)   HIP on MI355X
#   tiny      5.39e-07            6.03e-07   (the test prints it)
#   mid       4.54e-07            4.65e-07
#   full      7.68e-07            1.30e-06
#   ctx128    4.42e-07            4.63e-07   (test_the_longest_context_and_the_smallest_shapes; its e32 is computed by the test)
GATE_FACTOR = 4.0

_ENC = {}


def encoder(name):
    """one encoder per configuration with the fixture's weights, shared by the tests (do not load or close it)"""
    from oakink2_tamf_amd.model.text_encoder import HipClipTextEncoder

    if name not in _ENC:
        c = R.case(name)
        enc = HipClipTextEncoder(c["cfg"])
        enc.load_state_dict(c["sd"])
        _ENC[name] = enc
    return _ENC[name]


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", ["tiny", "mid", "full"])
def test_parity_with_the_float64_restatement(name):
    fix = load_golden(f"textenc_{name}.npz")
    out = encoder(name).encode_tokens(fix["ids"]).cpu().numpy()
    assert out.shape == fix["out64"].shape and out.dtype == np.float32 and np.isfinite(out).all()
    err = float(np.abs(out.astype(np.float64) - fix["out64"]).max() / np.abs(fix["out64"]).max())
    e32 = float(fix["e32"])
    print(f"textenc parity {name}: HIP {err:.3e}, CPU float32 e32 {e32:.3e}, gate {GATE_FACTOR * e32:.3e}")
    assert err <= GATE_FACTOR * e32


def test_the_longest_context_and_the_smallest_shapes():
    """context_length 128 - prompts of more than 80 rows put the attention kernel's K / V / score panels above 64 KiB of LDS, which
    has to be allowed per kernel - with one layer, one head and the narrowest projection (a 16-column tile tail).  The reference and
    e32 are computed here (the model is small); the gate is the parity test's."""
    from oakink2_tamf_amd.model.text_encoder import HipClipTextEncoder

    cfg = dict(vocab_size=40, context_length=128, width=64, num_heads=1, num_layers=1, embed_dim=16)
    eot = [127, 80, 96, 0, 63, 79]
    sd, ids = R.seeded_state_dict(cfg, 311), R.seeded_ids(cfg, eot, 411)
    out64 = R.forward(sd, cfg, ids)
    e32 = R.float32_error(sd, cfg, ids, out64)
    enc = HipClipTextEncoder(cfg)
    enc.load_state_dict(sd)
    out = enc.encode_tokens(ids)
    alone = [bits(enc.encode_tokens(ids[b: b + 1]))[0] for b in range(len(eot))]
    enc.close()
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - out64).max() / np.abs(out64).max())
    print(f"textenc parity ctx128: HIP {err:.3e}, CPU float32 e32 {e32:.3e}, gate {GATE_FACTOR * e32:.3e}")
    assert 0 < e32 < 1e-5 and err <= GATE_FACTOR * e32
    assert np.array_equal(np.stack(alone), bits(out))  # (alone, the short prompts run with small panels: the same bits)


@pytest.mark.parametrize("name", ["tiny", "mid", "full"])
def test_batch_invariance_bit_for_bit(name):
    enc, ids = encoder(name), R.case(name)["ids"]
    B = ids.shape[0]
    batch = bits(enc.encode_tokens(ids))
    for b in range(B):  # each prompt alone
        assert np.array_equal(bits(enc.encode_tokens(ids[b: b + 1]))[0], batch[b]), b
    assert np.array_equal(bits(enc.encode_tokens(ids[::-1].copy()))[::-1], batch)  # reversed order
    # beside prompts of other lengths: the longest in front of every short one, then odd subsets
    order = [int(np.argmax(R.EOT_POSITIONS[name]))] + [b for b in range(B) if R.EOT_POSITIONS[name][b] < 16]
    assert np.array_equal(bits(enc.encode_tokens(ids[order])), batch[order])
    for sub in ([1, 7], [3, 2, 1], [10, 0, 4, 0, 9]):
        assert np.array_equal(bits(enc.encode_tokens(ids[sub])), batch[sub]), sub


@pytest.mark.parametrize("name", ["tiny", "full"])
def test_ids_behind_the_eot_position_change_no_bit(name):
    enc, c = encoder(name), R.case(name)
    ids, V = c["ids"], c["cfg"]["vocab_size"]
    want = bits(enc.encode_tokens(ids))
    rng = np.random.default_rng(9)
    other = ids.copy()
    for b, e in enumerate(R.EOT_POSITIONS[name]):
        # arbitrary valid ids, the row's own maximum included (the first one counts); the all-zero row has no smaller id to offer
        other[b, e + 1:] = rng.integers(0, int(ids[b, e]) + 1, ids.shape[1] - e - 1)
    assert (other != ids).sum() > ids.shape[1] and other.max() == V - 1
    assert np.array_equal(np.argmax(other, axis=1), R.EOT_POSITIONS[name])
    assert np.array_equal(bits(enc.encode_tokens(other)), want)


def test_of_two_eot_ids_the_first_counts():
    enc, c = encoder("mid"), R.case("mid")
    V = c["cfg"]["vocab_size"]
    b = R.EOT_POSITIONS["mid"].index(5)
    one = c["ids"][b: b + 1].copy()
    two = one.copy()
    two[0, 9], two[0, 23] = V - 1, V - 1
    assert int(np.argmax(two[0])) == 5
    assert np.array_equal(bits(enc.encode_tokens(two)), bits(enc.encode_tokens(one)))
    late = one.copy()
    late[0, 5] = V - 2  # now the later one is the only maximum: another row is read
    late[0, 9] = V - 1
    assert not np.array_equal(bits(enc.encode_tokens(late)), bits(enc.encode_tokens(one)))


def test_round_fp16_equals_weights_rounded_on_the_host():
    from oakink2_tamf_amd.model.text_encoder import HipClipTextEncoder

    cfg, ids = R.CONFIGS["mid"], R.case("mid")["ids"]
    raw = R.seeded_state_dict(cfg, R.WEIGHT_SEED["mid"], fp16=False)
    assert any(not np.array_equal(v.astype(np.float16).astype(np.float32), v) for k, v in raw.items() if R.is_fp16_key(k))
    outs = []
    for sd, flag in ((raw, True), (R.round_fp16(raw), False), (raw, False)):
        enc = HipClipTextEncoder(cfg, round_fp16=flag)
        enc.load_state_dict(sd)
        outs.append(bits(enc.encode_tokens(ids)))
        enc.close()
    assert np.array_equal(outs[0], outs[1])
    assert not np.array_equal(outs[0], outs[2])
    assert np.array_equal(outs[0], bits(encoder("mid").encode_tokens(ids)))  # (the fixture's weights are the rounded ones)


def test_error_paths():
    from oakink2_tamf_amd.model import text_encoder as T

    enc, c = encoder("tiny"), R.case("tiny")
    bad = c["ids"].copy()
    bad[3, 9] = c["cfg"]["vocab_size"]  # behind the row's EOT position: still refused
    with pytest.raises(T.TextEncoderError, match=r"tokens\[3\]\[9\] = 64 outside \[0, 64\)"):
        enc.encode_tokens(bad)
    bad[3, 9] = -1
    with pytest.raises(T.TextEncoderError, match=r"tokens\[3\]\[9\] = -1"):
        enc.encode_tokens(bad)
    with pytest.raises(ValueError, match="expected integers of shape"):
        enc.encode_tokens(c["ids"][:, :8])
    # the library itself: a workspace one byte short, and encode on a model that was never finalised
    lib, ids = enc._lib, np.ascontiguousarray(c["ids"][:2])
    need = int(lib.tamf_textenc_workspace_bytes(enc._model, 2, int((T.eot_positions(ids) + 1).sum())))
    ws = torch.empty(need // 4, dtype=torch.float32, device=enc.device)
    out = torch.empty((2, enc.out_dim), dtype=torch.float32, device=enc.device)
    rc = lib.tamf_textenc_encode(enc._model, ids.ctypes.data, 2, out.data_ptr(), ws.data_ptr(), need - 1, None)
    assert rc == -1 and "workspace of" in lib.tamf_textenc_last_error().decode()
    assert lib.tamf_textenc_encode(enc._model, ids.ctypes.data, 2, out.data_ptr(), ws.data_ptr(), need, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), bits(enc.encode_tokens(ids)))
    fresh = T.HipClipTextEncoder(c["cfg"])
    with pytest.raises(T.TextEncoderError, match="no weights loaded"):
        fresh.encode_tokens(ids)
    rc = lib.tamf_textenc_encode(fresh._model, ids.ctypes.data, 2, out.data_ptr(), ws.data_ptr(), need, None)
    assert rc == -2 and "not finalised" in lib.tamf_textenc_last_error().decode()
    with pytest.raises(T.TextEncoderError, match="missing keys"):
        fresh.load_state_dict({k: v for k, v in c["sd"].items() if k != "positional_embedding"})
    fresh.close()


def test_embed_text_end_to_end(tmp_path):
    """the launcher on a cache dict, a seeded mid-size checkpoint written by torch.save and the synthetic vocabulary; the sampler's
    own loader reads the table, which equals encode_text called directly"""
    from oakink2_tamf_amd.launch.sample import load_text_embeddings
    from oakink2_tamf_amd.model.clip_tokenizer import ClipTokenizer
    from oakink2_tamf_amd.model.text_encoder import HipClipTextEncoder

    cfg = dict(R.CONFIGS["mid"], vocab_size=512 + 41 + 2)  # the synthetic vocabulary's size
    sd = R.seeded_state_dict(cfg, 77)
    ckpt, cfg_yml, cache, out = tmp_path / "tower.pt", tmp_path / "tower.yml", tmp_path / "cache.pkl", tmp_path / "emb" / "text.pkl"
    torch.save({"state_dict": {"clip_model." + k: torch.from_numpy(v) for k, v in sd.items()}}, ckpt)
    cfg_yml.write_text("".join(f"{k}: {v}\n" for k, v in cfg.items()))
    texts = ["Hold the cup.", "open the bottle", "pour the bottle with the right hand and hold the cup with the left hand to open the other bottle's top", "Hold the cup.",
             "hand", "cup &amp; bottle 42!!"]
    with open(cache, "wb") as f:
        pickle.dump({"interaction_segment_text_list": texts}, f)
    r = subprocess.run([sys.executable, "-m", "oakink2_tamf_amd.launch.embed_text", "--text_encoder.ckpt", str(ckpt), "--text_encoder.vocab", BPE,
                        "--text_encoder.cfg", str(cfg_yml), "--data.cache_dict_filepath", str(cache), "--out", str(out), "--batch_size", "2"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=PKG_PARENT), timeout=300)
    assert r.returncode == 0, r.stderr
    assert "5 prompts (1 truncated)" in r.stdout
    table = load_text_embeddings(str(out))
    assert set(table) == set(texts)
    enc = HipClipTextEncoder(cfg)
    enc.load_state_dict(sd)
    direct = enc.encode_text(sorted(set(texts)), ClipTokenizer(BPE), max_text_len=20).cpu().numpy()
    enc.close()
    for t, e in zip(sorted(set(texts)), direct):
        assert table[t].shape == (cfg["embed_dim"],) and table[t].dtype == np.float32 and np.isfinite(table[t]).all()
        assert np.array_equal(table[t].view(np.uint32), e.view(np.uint32)), t
    assert len({table[t].tobytes() for t in table}) == 5
