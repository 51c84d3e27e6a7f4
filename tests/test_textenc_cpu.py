"""CPU: the host side of the native text encoder - the references of the GPU tests (the float64 restatement pinned to its committed
fixtures and to a torch.nn assembly of the same model, the causal-mask properties the packed-row design rests on), the library's
description and surface, its host-side error paths through ctypes, the state-dict mapping and the embed_text launcher's dry run."""
import ctypes
import json
import os
import pickle
import re
import subprocess
import sys
from ctypes import POINTER, c_int64, c_void_p

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG_PARENT, ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import textenc_restatement as R  # noqa: E402

BPE = os.path.join(GOLDEN, "clip_bpe_synthetic.txt")
TAMF_ERR_INVALID, TAMF_ERR_STATE, TAMF_ERR_MISSING, TAMF_ERR_RANGE = -1, -2, -4, -6


def test_status_codes_are_the_headers():
    with open(os.path.join(ROOT, "include", "tamf_hip.h")) as f:
        hdr = f.read()
    got = {k: int(v) for k, v in re.findall(r"\b(TAMF_ERR_[A-Z]+)\s*=\s*(-?\d+)", hdr)}
    assert (got["TAMF_ERR_INVALID"], got["TAMF_ERR_STATE"], got["TAMF_ERR_MISSING"], got["TAMF_ERR_RANGE"]) == \
        (TAMF_ERR_INVALID, TAMF_ERR_STATE, TAMF_ERR_MISSING, TAMF_ERR_RANGE)


@pytest.mark.parametrize("name", ["tiny", "mid", "full"])
def test_the_restatement_reproduces_the_committed_fixture(name):
    """float64 against float64 of the same program: what differs between two machines is the BLAS's summation order, about 2^-29 of
    the float32 noise e32 - gated at e32 / 1000 (relative to max |out|), as the point encoder's fixtures are"""
    fix, c = load_golden(f"textenc_{name}.npz"), R.case(name)
    assert int(fix["weight_seed"]) == R.WEIGHT_SEED[name] and R.state_checksum(c["sd"]) == str(fix["state_checksum"])
    assert np.array_equal(fix["ids"], c["ids"]) and fix["ids"].dtype == np.int32
    got = R.forward(c["sd"], c["cfg"], c["ids"])
    assert got.dtype == np.float64 and got.shape == fix["out64"].shape == (len(R.EOT_POSITIONS[name]), c["cfg"]["embed_dim"])
    err = float(np.abs(got - fix["out64"]).max() / np.abs(fix["out64"]).max())
    print(f"{name}: restatement against fixture {err:.3e}, e32 = {float(fix['e32']):.3e}, max|out| = {np.abs(got).max():.2f}")
    assert 0 < float(fix["e32"]) < 1e-5 and err <= float(fix["e32"]) / 1000 and 1.0 < np.abs(got).max() < 10.0


@pytest.mark.parametrize("name", ["tiny", "mid", "full"])
def test_the_fixture_prompts_cover_the_edges(name):
    cfg, eot = R.CONFIGS[name], R.EOT_POSITIONS[name]
    ctx = cfg["context_length"]
    assert {e for e in (0, 1, 2, 15, 16, 17, 21, ctx - 1) if e < ctx} <= set(eot) and max(eot) == ctx - 1
    ids = R.case(name)["ids"]
    assert not ids[eot.index(0)].any()  # the all-zero id row
    first = np.cumsum([0] + [e + 1 for e in eot])  # first packed row of every prompt, and the total
    assert any(a % R.GEMM_TILE and a // R.GEMM_TILE != (b - 1) // R.GEMM_TILE for a, b in zip(first, first[1:])), "no prompt straddles a tile boundary"
    assert first[-1] > R.GEMM_TILE
    # the weights are fp16-representable where the reference keeps fp16, and not elsewhere
    sd = R.case(name)["sd"]
    for k, v in sd.items():
        assert v.dtype == np.float32 and np.array_equal(v.astype(np.float16).astype(np.float32), v) == R.is_fp16_key(k), k


@pytest.mark.parametrize("name", ["tiny", "mid", "full"])
def test_the_definition_agrees_with_a_torch_nn_assembly(name):
    """the numpy restatement against torch.nn.Embedding / MultiheadAttention / LayerNorm / Linear loaded (strictly) from the same
    state dict, both in float64: two summation orders of the same sums.  Gate: e32 / 1000 relative to max |out|, as above.  And the
    float32 assembly - the unit of the GPU gate - stays inside the GPU gate of 4 * e32 on this machine too."""
    fix, c = load_golden(f"textenc_{name}.npz"), R.case(name)
    with torch.no_grad():
        got = R.torch_tower(c["sd"], c["cfg"], torch.float64)(c["ids"]).numpy()
    scale, e32 = np.abs(fix["out64"]).max(), float(fix["e32"])
    err = float(np.abs(got - fix["out64"]).max() / scale)
    here32 = R.float32_error(c["sd"], c["cfg"], c["ids"], fix["out64"])
    print(f"{name}: torch.nn float64 against the restatement {err:.3e}; float32 here {here32:.3e}, fixture e32 {e32:.3e}")
    assert err <= e32 / 1000
    assert 0 < here32 <= 4 * e32


@pytest.mark.parametrize("name", ["tiny", "mid"])
def test_the_causal_mask_makes_the_eot_row_independent_of_what_follows(name):
    c = R.case(name)
    cfg, sd, ids = c["cfg"], c["sd"], c["ids"]
    full = R.forward(sd, cfg, ids)
    rng = np.random.default_rng(5)
    for b, e in enumerate(R.EOT_POSITIONS[name]):
        # only rows <= eot: the same EOT row, to float64 rounding (the matmuls see other shapes; no term is added or dropped)
        short = R.forward(sd, cfg, ids[b: b + 1], length=e + 1)
        assert np.abs(short - full[b]).max() <= 1e-12
        # other ids behind the EOT position: nothing changes at all (ids below the row's maximum keep the argmax where it is)
        if e + 1 < cfg["context_length"]:
            other = ids[b: b + 1].copy()
            other[0, e + 1:] = rng.integers(0, max(int(ids[b, e]), 1), cfg["context_length"] - e - 1)
            assert int(np.argmax(other[0])) == e
            assert np.array_equal(R.forward(sd, cfg, other), R.forward(sd, cfg, ids[b: b + 1]))  # (the same shapes: the same bits)


def test_library_description():
    from oakink2_tamf_amd import _lib

    with open(os.path.join(ROOT, "include", "tamf_textenc.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert set(re.findall(r"\b(tamf_[a-z0-9_]+)\s*\(", hdr)) == set(_lib.TEXTENC_EXPORTS) and len(set(_lib.TEXTENC_EXPORTS)) == len(_lib.TEXTENC_EXPORTS)
    assert not set(_lib.TEXTENC_EXPORTS) & set(_lib.EXPORTS + _lib.EVAL_EXPORTS + _lib.HOOK_EXPORTS + _lib.MANO_EXPORTS + _lib.POINTENC_EXPORTS)
    # no other library's sources: tamf_f32_tower.h and tamf_weights.h are common ground of the two encoders, like tamf_device.h
    assert _lib.TEXTENC.sources == ["tamf_device.h", "tamf_f32_tower.h", "tamf_textenc.h", "tamf_textenc.hip", "tamf_weights.h"]
    assert not [s for lib in _lib.LIBRARIES for s in lib.sources if s in ("tamf_f32_tower.h", "tamf_weights.h")]
    assert not [s for s in _lib.TEXTENC.sources if s.startswith("tamf_pointenc")] and not [s for s in _lib.POINTENC.sources if s.startswith("tamf_textenc")]
    assert not [s for lib in _lib.LIBRARIES + _lib.PREPROCESSING for s in lib.sources if s.startswith("tamf_textenc")]
    assert _lib.LIBRARIES == (_lib.SAMPLER, _lib.EVAL, _lib.MANO) and _lib.PREPROCESSING == (_lib.POINTENC,) and _lib.TEXT_PREPROCESSING == (_lib.TEXTENC,)
    assert _lib.TEXTENC.paths == [_lib.TEXTENC_LIB_PATH] and len(_lib.EXPORTS) == 27
    assert len({lib.stamp_path for lib in _lib.LIBRARIES + _lib.PREPROCESSING + _lib.TEXT_PREPROCESSING}) == 5
    assert len(_lib.TEXTENC.kernels) == 4
    path = _lib.TEXTENC.build()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    syms = {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln}
    assert {s for s in syms if s.startswith("tamf_")} == set(_lib.TEXTENC_EXPORTS)
    lib = _lib.load_textenc()
    for s in _lib.TEXTENC_EXPORTS:
        getattr(lib, s)


def _create(lib, cfg_cls, **over):
    cfg = dict(R.CONFIGS["tiny"], **over)
    model = c_void_p()
    rc = lib.tamf_textenc_model_create(ctypes.byref(cfg_cls(**cfg)), ctypes.byref(model))
    return rc, model


def _load(lib, model, key, a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return lib.tamf_textenc_load_weight(model, key.encode(), a.ctypes.data, a.ndim, (c_int64 * max(a.ndim, 1))(*a.shape))


def test_host_side_errors_need_no_gpu():
    from oakink2_tamf_amd.model import text_encoder as T

    lib = T._bind()
    err = lambda: lib.tamf_textenc_last_error().decode()  # noqa: E731
    for over, word in ((dict(vocab_size=1), "vocab_size"), (dict(context_length=1), "context_length"), (dict(context_length=129), "context_length"),
                       (dict(width=96), "width"), (dict(width=1088, num_heads=17), "width"), (dict(num_heads=2), "num_heads"),
                       (dict(num_layers=0), "num_layers"), (dict(embed_dim=40), "embed_dim"), (dict(embed_dim=1040), "embed_dim"), (dict(embed_dim=0), "embed_dim")):
        rc, model = _create(lib, T._Config, **over)
        assert rc == TAMF_ERR_INVALID and not model.value and word in err(), (over, err())
    for ok in (dict(context_length=2), dict(context_length=128), dict(width=1024, num_heads=16), dict(embed_dim=16), dict(embed_dim=1024), dict(vocab_size=2)):
        rc, model = _create(lib, T._Config, **ok)
        assert rc == 0 and model.value, (ok, err())
        assert lib.tamf_textenc_destroy(model) == 0
    rc, model = _create(lib, T._Config)
    assert rc == 0
    sd = R.case("tiny")["sd"]
    assert _load(lib, model, "visual.proj", np.zeros((4, 4))) == TAMF_ERR_INVALID and "unknown key 'visual.proj'" in err()
    assert _load(lib, model, "text_projection", np.zeros((32, 64))) == TAMF_ERR_INVALID and "expected shape (64, 32), got (32, 64)" in err()
    assert _load(lib, model, "ln_final.bias", np.zeros((64, 1))) == TAMF_ERR_INVALID
    # nothing to encode with, nothing to size: encode before finalize is a state error, a missing tensor is named
    tokens = np.zeros((1, 16), np.int32)
    assert lib.tamf_textenc_encode(model, tokens.ctypes.data, 1, c_void_p(16), c_void_p(16), 1 << 20, None) == TAMF_ERR_STATE and "not finalised" in err()
    for k, v in sd.items():
        if k != "transformer.resblocks.1.mlp.c_proj.bias":
            assert _load(lib, model, k, v) == 0, err()
    assert lib.tamf_textenc_finalize(model, 1) == TAMF_ERR_MISSING and "transformer.resblocks.1.mlp.c_proj.bias" in err()
    bad = sd["ln_final.weight"].copy()
    bad[3] = np.inf
    assert _load(lib, model, "transformer.resblocks.1.mlp.c_proj.bias", sd["transformer.resblocks.1.mlp.c_proj.bias"]) == 0
    assert _load(lib, model, "ln_final.weight", bad) == 0
    assert lib.tamf_textenc_finalize(model, 1) == TAMF_ERR_RANGE and "ln_final.weight" in err()
    big = sd["text_projection"].copy()
    big[0, 0] = 1e6  # finite, beyond fp16
    assert _load(lib, model, "ln_final.weight", sd["ln_final.weight"]) == 0 and _load(lib, model, "text_projection", big) == 0
    assert lib.tamf_textenc_finalize(model, 1) == TAMF_ERR_RANGE and "fp16 range" in err()
    assert lib.tamf_textenc_destroy(model) == 0
    # a complete, finite set: finalize seals the model whether or not there is a device to upload to - no tensor is taken afterwards
    rc, model = _create(lib, T._Config)
    for k, v in sd.items():
        assert _load(lib, model, k, v) == 0
    rc = lib.tamf_textenc_finalize(model, 1)
    assert rc == 0 if torch.cuda.is_available() else rc < 0
    assert _load(lib, model, "ln_final.bias", sd["ln_final.bias"]) == TAMF_ERR_STATE and "finalised" in err()
    assert lib.tamf_textenc_finalize(model, 1) == TAMF_ERR_STATE
    assert lib.tamf_textenc_workspace_bytes(model, 0, 0) == 0 and lib.tamf_textenc_workspace_bytes(model, 2, 1) == 0
    assert lib.tamf_textenc_workspace_bytes(model, 2, 33) == 0  # more rows than two contexts hold
    assert lib.tamf_textenc_workspace_bytes(model, 2, 20) >= 4 * (20 * 64 * 10 + 2 * 64)
    assert lib.tamf_textenc_workspace_bytes(None, 1, 1) == 0
    assert lib.tamf_textenc_destroy(model) == 0 and lib.tamf_textenc_destroy(None) == 0


def test_state_dict_mapping():
    from oakink2_tamf_amd.model.text_encoder import DEFAULT_CFG, expected_shapes, is_fp16_key, make_cfg, map_state_dict

    cfg = make_cfg(R.CONFIGS["mid"])
    sd = R.case("mid")["sd"]
    assert {k: v.shape for k, v in sd.items()} == expected_shapes(cfg) and list(sd) != sorted(sd)
    assert all(is_fp16_key(k) == R.is_fp16_key(k) for k in sd)
    ckpt = {"clip_model." + k: v for k, v in sd.items()}
    ckpt.update({"clip_model.visual.conv1.weight": np.zeros(3), "logit_scale": np.zeros(()), "context_length": np.int64(77)})
    got, missing, ignored = map_state_dict(ckpt, cfg)
    assert set(got) == set(sd) and not missing and sorted(ignored) == ["context_length", "logit_scale", "visual.conv1.weight"]
    del ckpt["clip_model.text_projection"]
    assert map_state_dict(ckpt, cfg)[1] == ["text_projection"]
    full = expected_shapes(make_cfg())
    assert make_cfg() == DEFAULT_CFG == R.CONFIGS["full"] and 63.0e6 < sum(int(np.prod(s)) for s in full.values()) < 63.6e6
    assert 37.5e6 < sum(int(np.prod(s)) for k, s in full.items() if "resblocks" in k) < 38.0e6  # what a call streams
    with pytest.raises(KeyError, match="unknown field"):
        make_cfg({"heads": 8})


def test_encoder_needs_a_gpu():
    from oakink2_tamf_amd.hip_backend import TamfError
    from oakink2_tamf_amd.model.text_encoder import HipClipTextEncoder

    if torch.cuda.is_available():
        HipClipTextEncoder(R.CONFIGS["tiny"]).close()
    else:
        with pytest.raises(TamfError, match="no CPU fallback"):
            HipClipTextEncoder(R.CONFIGS["tiny"])


def _run(*args):
    env = dict(os.environ, PYTHONPATH=PKG_PARENT)
    return subprocess.run([sys.executable, "-m", "oakink2_tamf_amd.launch.embed_text", *args], capture_output=True, text=True, env=env, timeout=120)


def test_embed_text_dry_run(tmp_path):
    cache = tmp_path / "cache.pkl"
    texts = ["Hold the cup.", "pour the bottle with the right hand and hold the cup with the left hand to open other", "Hold the cup.", "open the bottle"]
    with open(cache, "wb") as f:
        pickle.dump({"interaction_segment_text_list": texts, "interaction_segment_key_list": list(range(4))}, f)
    r = _run("--text_encoder.vocab", BPE, "--data.cache_dict_filepath", str(cache), "--out", str(tmp_path / "o" / "t.pkl"), "--dry_run")
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert [p["text"] for p in d["prompts"]] == sorted(set(texts)) and d["out"] == str(tmp_path / "o" / "t.pkl") and not (tmp_path / "o").exists()
    assert d["cfg"] == R.CONFIGS["full"] and d["vocab_size"] == 512 + 41 + 2 and d["max_text_len"] == 20 and d["round_fp16"] is True
    by = {p["text"]: p for p in d["prompts"]}
    assert by["Hold the cup."] == {"text": "Hold the cup.", "tokens": 6, "truncated": False}  # SOT hold the cup . EOT
    assert by[texts[1]]["tokens"] > 22 and by[texts[1]]["truncated"] and not by["open the bottle"]["truncated"]
    r = _run("--text_encoder.vocab", BPE, "--data.cache_dict_filepath", str(cache), "--dry_run", "--max_text_len", "3", "--no_round_fp16")
    d = json.loads(r.stdout)
    assert r.returncode == 0 and [p["truncated"] for p in d["prompts"]] == [True, False, True] and d["round_fp16"] is False
    # prompts from a file keep their order; a non-ASCII prompt is an error that names it; so is a missing vocabulary or checkpoint
    tf = tmp_path / "prompts.txt"
    tf.write_text("open the bottle\n\nHold the cup.\nopen the bottle\n")
    r = _run("--text_encoder.vocab", BPE, "--text_file", str(tf), "--dry_run")
    assert r.returncode == 0 and [p["text"] for p in json.loads(r.stdout)["prompts"]] == ["open the bottle", "Hold the cup."]
    tf.write_text("open the café\n", encoding="utf-8")
    r = _run("--text_encoder.vocab", BPE, "--text_file", str(tf), "--dry_run")
    assert r.returncode != 0 and "caf" in r.stderr and "ASCII" in r.stderr
    assert _run("--text_file", str(tf), "--dry_run").returncode != 0
    tf.write_text("open the bottle\n")
    r = _run("--text_encoder.vocab", BPE, "--text_file", str(tf))
    assert r.returncode != 0 and "--text_encoder.ckpt is required" in r.stderr
    # the shell wrapper
    r = subprocess.run(["bash", os.path.join(ROOT, "script", "embed_text.sh"), "-n", "w.pt", "v.txt.gz", "--dry_run"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "python -m oakink2_tamf_amd.launch.embed_text --text_encoder.ckpt w.pt --text_encoder.vocab v.txt.gz --dry_run" in r.stdout
    assert subprocess.run(["bash", os.path.join(ROOT, "script", "embed_text.sh"), "w.pt"], capture_output=True, text=True, timeout=60).returncode == 2


def test_the_table_round_trips_through_the_samplers_loader(tmp_path):
    from oakink2_tamf_amd.launch.embed_text import save_table
    from oakink2_tamf_amd.launch.sample import load_text_embeddings

    emb = np.random.default_rng(2).normal(size=(2, 512)).astype(np.float32)
    path = str(tmp_path / "sub" / "t.pkl")
    save_table(path, ["a", "b"], emb)
    got = load_text_embeddings(path)
    assert list(got) == ["a", "b"] and all(got[k].dtype == np.float32 and got[k].shape == (512,) for k in got) and np.array_equal(got["b"], emb[1])
    emb[1, 7] = np.nan
    with pytest.raises(ValueError, match="'b'"):
        save_table(path, ["a", "b"], emb)
