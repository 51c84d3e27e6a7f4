"""CPU: the host side of the native point encoder - BatchNorm folding (libtamf_pointenc.so's host entry point), the checkpoint
prefix mapping, the library's surface, the embed_objects launcher's dry run and cloud preparation, and the embedding file format;
and the references of the GPU tests themselves: the plain-torch restatement pinned to the reference's captured outputs, the sweep
cases of tests/test_pointenc_edges_gpu.py and the host emulations of FPS and grouping."""
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import PKG_PARENT, ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import pointenc_fixture as F  # noqa: E402


@pytest.mark.parametrize("case", ["tiny", "mid"])
def test_bn_folding_matches_the_unfolded_float64_restatement(case):
    """relu(BN(conv(x))) in float64 from the unfolded parameters against relu(conv'(x)) with the folded float32 weights, evaluated
    in float64: what is left is the one rounding of each folded weight and bias to float32, <= 2^-24 relative per term, i.e.
    2^-24 * (sum_i |w'_i x_i| + |b'|) per output"""
    from oakink2_tamf_amd.model.point_encoder import fold_bn

    cfg = F.CASES[case][0]
    sd = F.seeded_state_dict(cfg, 11)
    C = cfg["point_dims"]
    p = "encoder.first_conv."
    w, b = fold_bn(sd[p + "0.weight"], sd[p + "0.bias"], sd[p + "1.weight"], sd[p + "1.bias"], sd[p + "1.running_mean"], sd[p + "1.running_var"],
                   ld_out=(C + 3) // 4 * 4)
    assert w.shape == (128, (C + 3) // 4 * 4) and w.dtype == np.float32 and not w[:, C:].any()
    x = np.random.default_rng(0).normal(size=(200, C)).astype(np.float32).astype(np.float64)
    want = F.pointnet_first_layer(sd, x, torch.float64).numpy()
    w64, b64 = w[:, :C].astype(np.float64), b.astype(np.float64)
    got = np.maximum(x @ w64.T + b64, 0.0)
    bound = 2.0 ** -24 * (np.abs(x) @ np.abs(w64).T + np.abs(b64)) + 1e-15
    assert (np.abs(got - want) <= bound).all()
    # the 512 -> 512 layer folds the same way (no padding)
    p = "encoder.second_conv."
    w2, b2 = fold_bn(sd[p + "0.weight"], sd[p + "0.bias"], sd[p + "1.weight"], sd[p + "1.bias"], sd[p + "1.running_mean"], sd[p + "1.running_var"])
    s = sd[p + "1.weight"].astype(np.float64) / np.sqrt(sd[p + "1.running_var"].astype(np.float64) + 1e-5)
    assert np.array_equal(w2, (s[:, None] * sd[p + "0.weight"][:, :, 0].astype(np.float64)).astype(np.float32))
    assert np.array_equal(b2, ((sd[p + "0.bias"].astype(np.float64) - sd[p + "1.running_mean"]) * s + sd[p + "1.bias"]).astype(np.float32))


def test_bn_folding_rejects_bad_statistics():
    from oakink2_tamf_amd.model.point_encoder import PointEncoderError, fold_bn

    one = np.ones(4, np.float32)
    w = np.ones((4, 3), np.float32)
    with pytest.raises(PointEncoderError, match="running_var"):
        fold_bn(w, one, one, one, one, -one)
    bad = one.copy()
    bad[2] = np.nan
    with pytest.raises(PointEncoderError, match="channel 2"):
        fold_bn(w, one, bad, one, one, one)


def test_checkpoint_prefix_mapping_reports_missing_and_unexpected_keys():
    from oakink2_tamf_amd.model.point_encoder import PREFIX, expected_shapes, make_cfg, map_checkpoint

    cfg = make_cfg(F.CASES["tiny"][0])
    sd = F.seeded_state_dict(cfg, 1)
    assert {k: v.shape for k, v in sd.items()} == expected_shapes(cfg)
    ckpt = {PREFIX + k: v for k, v in sd.items()}
    ckpt[PREFIX + "encoder.first_conv.1.num_batches_tracked"] = np.int64(7)  # a counter, no weight
    ckpt["module.llm.embed.weight"] = np.zeros(3)                            # another module of the checkpoint: dropped
    got, missing, unexpected = map_checkpoint(ckpt, cfg)
    assert set(got) == set(sd) and not missing and not unexpected
    del ckpt[PREFIX + "norm.bias"], ckpt[PREFIX + "blocks.blocks.0.attn.qkv.weight"]
    ckpt[PREFIX + "blocks.blocks.0.attn.qkv.bias"] = np.zeros(3)
    ckpt[PREFIX + "cls_head.0.weight"] = np.zeros(3)
    got, missing, unexpected = map_checkpoint(ckpt, cfg)
    assert missing == ["blocks.blocks.0.attn.qkv.weight", "norm.bias"]
    assert sorted(unexpected) == ["blocks.blocks.0.attn.qkv.bias", "cls_head.0.weight"]
    assert set(got) == set(sd) - set(missing)
    # the default configuration is the reference's: 21.9 M parameters, output 768
    full = expected_shapes(make_cfg())
    assert 21.8e6 < sum(int(np.prod(s)) for s in full.values()) < 22.0e6 and make_cfg()["trans_dim"] * 2 == 768
    with pytest.raises(KeyError, match="unknown field"):
        make_cfg({"transdim": 384})


def test_header_exports_and_source_closure():
    from oakink2_tamf_amd import _lib

    with open(os.path.join(ROOT, "include", "tamf_pointenc.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert set(re.findall(r"\b(tamf_[a-z0-9_]+)\s*\(", hdr)) == set(_lib.POINTENC_EXPORTS) and len(set(_lib.POINTENC_EXPORTS)) == len(_lib.POINTENC_EXPORTS)
    assert not set(_lib.POINTENC_EXPORTS) & set(_lib.EXPORTS + _lib.EVAL_EXPORTS + _lib.HOOK_EXPORTS + _lib.MANO_EXPORTS)
    # no other library's sources: tamf_f32_tower.h and tamf_weights.h are common ground of the two encoders, like tamf_device.h
    assert _lib.POINTENC.sources == ["tamf_device.h", "tamf_f32_tower.h", "tamf_pointenc.h", "tamf_pointenc.hip", "tamf_weights.h"]
    assert not [s for lib in _lib.LIBRARIES for s in lib.sources if s in ("tamf_f32_tower.h", "tamf_weights.h")]
    assert not [s for s in _lib.TEXTENC.sources if s.startswith("tamf_pointenc")] and not [s for s in _lib.POINTENC.sources if s.startswith("tamf_textenc")]
    assert not [s for lib in _lib.LIBRARIES for s in lib.sources if s.startswith("tamf_pointenc")]
    assert _lib.POINTENC in _lib.PREPROCESSING and _lib.POINTENC.paths == [_lib.POINTENC_LIB_PATH]
    assert len({lib.stamp_path for lib in _lib.LIBRARIES + _lib.PREPROCESSING}) == 4
    path = _lib.POINTENC.build()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    syms = {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln}
    assert {s for s in syms if s.startswith("tamf_")} == set(_lib.POINTENC_EXPORTS)
    lib = _lib.load_pointenc()
    for s in _lib.POINTENC_EXPORTS:
        getattr(lib, s)


def test_encoder_needs_a_gpu():
    from oakink2_tamf_amd.hip_backend import TamfError
    from oakink2_tamf_amd.model.point_encoder import HipPointEncoder

    if torch.cuda.is_available():
        HipPointEncoder(F.CASES["tiny"][0]).close()
    else:
        with pytest.raises(TamfError, match="no CPU fallback"):
            HipPointEncoder(F.CASES["tiny"][0])


TAMF_ERR_INVALID, TAMF_ERR_STATE, TAMF_ERR_MISSING, TAMF_ERR_RANGE = -1, -2, -4, -6  # (include/tamf_hip.h; pinned by test_textenc_cpu.py)


def test_host_side_errors_need_no_gpu():
    """the library's host paths through ctypes, as tests/test_textenc_cpu.py pins the text tower's.  Unlike the text tower, the point
    encoder becomes final only with a successful upload: without a device it can still be loaded into."""
    import ctypes
    from ctypes import c_int64, c_void_p

    from oakink2_tamf_amd.model import point_encoder as P

    lib = P._bind()
    err = lambda: lib.tamf_pointenc_last_error().decode()  # noqa: E731
    cfg = F.CASES["tiny"][0]
    sd = F.seeded_state_dict(cfg, 1)

    def create(**over):
        model = c_void_p()
        return lib.tamf_pointenc_model_create(ctypes.byref(P._Config(**dict(cfg, **over))), ctypes.byref(model)), model

    def load(model, key, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        return lib.tamf_pointenc_load_weight(model, key.encode(), a.ctypes.data, a.ndim, (c_int64 * max(a.ndim, 1))(*a.shape))

    for over, word in ((dict(point_dims=4), "point_dims"), (dict(trans_dim=96), "trans_dim"), (dict(num_heads=3), "num_heads"), (dict(depth=0), "depth"),
                       (dict(num_group=1025), "num_group"), (dict(group_size=7), "group_size"), (dict(encoder_dims=40), "encoder_dims")):
        rc, model = create(**over)
        assert rc == TAMF_ERR_INVALID and not model.value and word in err(), (over, err())
    rc, model = create()
    assert rc == 0 and model.value
    assert load(model, "visual.proj", np.zeros((4, 4))) == TAMF_ERR_INVALID and err() == "unknown key 'visual.proj'"
    assert load(model, "encoder.first_conv.1.num_batches_tracked", np.zeros(())) == TAMF_ERR_INVALID and "unknown key" in err()
    assert load(model, "reduce_dim.weight", np.zeros((64, 128))) == TAMF_ERR_INVALID and err() == "reduce_dim.weight: expected shape (128, 64), got (64, 128)"
    assert load(model, "cls_token", np.zeros((128,))) == TAMF_ERR_INVALID and err() == "cls_token: expected shape (1, 1, 128), got (128)"
    assert lib.tamf_pointenc_load_weight(model, b"norm.bias", None, 1, (c_int64 * 1)(128)) == TAMF_ERR_INVALID and err() == "null argument"
    # nothing to encode with: encode before finalize is a state error; a missing tensor and a non-finite one are named by finalize
    enc = lib.tamf_pointenc_encode(model, c_void_p(16), c_void_p(16), c_void_p(16), 1, 250, c_void_p(16), c_void_p(16), 1 << 20, None)
    assert enc == TAMF_ERR_STATE and "not finalised" in err()
    for k, v in sd.items():
        if k != "blocks.blocks.1.mlp.fc2.bias":
            assert load(model, k, v) == 0, err()
    assert lib.tamf_pointenc_finalize(model) == TAMF_ERR_MISSING and err() == "missing key 'blocks.blocks.1.mlp.fc2.bias'"
    bad = sd["norm.weight"].copy()
    bad[3] = np.inf
    assert load(model, "blocks.blocks.1.mlp.fc2.bias", sd["blocks.blocks.1.mlp.fc2.bias"]) == 0 and load(model, "norm.weight", bad) == 0
    assert lib.tamf_pointenc_finalize(model) == TAMF_ERR_RANGE and err() == "norm.weight: holds a non-finite value"
    var = sd["encoder.first_conv.1.running_var"].copy()
    var[5] = -1.0  # finite, but BatchNorm cannot be folded
    assert load(model, "norm.weight", sd["norm.weight"]) == 0 and load(model, "encoder.first_conv.1.running_var", var) == 0
    assert lib.tamf_pointenc_finalize(model) == TAMF_ERR_RANGE and "BatchNorm channel 5" in err()
    assert lib.tamf_pointenc_encode(model, c_void_p(16), c_void_p(16), c_void_p(16), 1, 250, c_void_p(16), c_void_p(16), 1 << 20, None) == TAMF_ERR_STATE
    # a complete, finite set: final with the upload - where there is no device, finalize fails and the model still takes tensors
    assert load(model, "encoder.first_conv.1.running_var", sd["encoder.first_conv.1.running_var"]) == 0
    rc = lib.tamf_pointenc_finalize(model)
    if torch.cuda.is_available():
        assert rc == 0 and load(model, "norm.bias", sd["norm.bias"]) == TAMF_ERR_STATE and "finalised" in err()
        assert lib.tamf_pointenc_finalize(model) == TAMF_ERR_STATE and "finalised already" in err()
    else:
        assert rc < 0 and "hipMalloc" in err()
        assert load(model, "norm.bias", sd["norm.bias"]) == 0
        assert lib.tamf_pointenc_encode(model, c_void_p(16), c_void_p(16), c_void_p(16), 1, 250, c_void_p(16), c_void_p(16), 1 << 20, None) == TAMF_ERR_STATE
    G, M, D, E = cfg["num_group"], cfg["group_size"], cfg["trans_dim"], cfg["encoder_dims"]
    assert lib.tamf_pointenc_workspace_bytes(None, 1) == 0 and lib.tamf_pointenc_workspace_bytes(model, 0) == 0 and lib.tamf_pointenc_workspace_bytes(model, -3) == 0
    one, two = lib.tamf_pointenc_workspace_bytes(model, 1), lib.tamf_pointenc_workspace_bytes(model, 2)
    assert one >= 4 * (G * M * (4 + 128 + 256 + 512 + E) + (G + 1) * 10 * D) and one % 16 == 0 and one < two <= 2 * one
    assert lib.tamf_pointenc_destroy(model) == 0 and lib.tamf_pointenc_destroy(None) == 0


def _run(*args):
    env = dict(os.environ, PYTHONPATH=PKG_PARENT)
    return subprocess.run([sys.executable, "-m", "oakink2_tamf_amd.launch.embed_objects", *args], capture_output=True, text=True, env=env, timeout=120)


def test_embed_objects_dry_run(tmp_path):
    pc = tmp_path / "pc"
    pc.mkdir()
    for oid in ("O02@0015@00001", "C12001"):
        np.savez(pc / f"{oid}.npz", point=np.zeros((8192, 3), np.float32))
    r = _run("--data.obj_pointcloud_prefix", str(pc), "--out_dir", str(tmp_path / "emb"), "--dry_run", "--color", "0.5,0.5,0.5", "--seed", "3")
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert [w["obj_id"] for w in d["work"]] == ["C12001", "O02@0015@00001"] and d["color"] == [0.5, 0.5, 0.5] and d["seed"] == 3 and not d["pc_norm"]
    assert d["work"][0]["embedding"] == str(tmp_path / "emb" / "C12001.pt") and not (tmp_path / "emb").exists()
    assert d["cfg"] == dict(point_dims=6, trans_dim=384, depth=12, num_heads=6, num_group=512, group_size=32, encoder_dims=256, npoints=8192)
    r = _run("--data.obj_pointcloud_prefix", str(pc), "--obj_ids", "C12001", "--dry_run")
    assert r.returncode == 0 and [w["obj_id"] for w in json.loads(r.stdout)["work"]] == ["C12001"]
    r = _run("--data.obj_pointcloud_prefix", str(pc), "--obj_ids", "C12001,nope", "--dry_run")
    assert r.returncode != 0 and "nope.npz not found" in r.stderr
    # the reference's yaml layout is accepted as --point_encoder.cfg
    y = tmp_path / "pe.yaml"
    y.write_text("model : {\n  NAME: PointTransformer,\n  trans_dim: 128,\n  depth: 2,\n  drop_path_rate: 0.1,\n  cls_dim: 40,\n  num_heads: 2,\n"
                 "  group_size: 8,\n  num_group: 17,\n  encoder_dims: 64,\n  point_dims: 3,\n  use_max_pool: false\n}\nnpoints: 250\n")
    r = _run("--data.obj_pointcloud_prefix", str(pc), "--point_encoder.cfg", str(y), "--dry_run")
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)["cfg"] == dict(F.CASES["tiny"][0], npoints=250)
    # the shell wrapper
    r = subprocess.run(["bash", os.path.join(ROOT, "script", "embed_objects.sh"), "-n", "w.pt", "--pc_norm"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "python -m oakink2_tamf_amd.launch.embed_objects --point_encoder.ckpt w.pt --pc_norm" in r.stdout
    assert subprocess.run(["bash", os.path.join(ROOT, "script", "embed_objects.sh")], capture_output=True, text=True, timeout=60).returncode == 2


def test_prepare_cloud():
    from oakink2_tamf_amd.launch.embed_objects import prepare_cloud

    rng = np.random.default_rng(0)
    xyz, rgb = rng.normal(size=(50, 3)).astype(np.float32), rng.uniform(size=(50, 3)).astype(np.float32)
    assert np.array_equal(prepare_cloud(np.concatenate([xyz, rgb], 1), 6, None, False), np.concatenate([xyz, rgb], 1))
    assert np.array_equal(prepare_cloud(np.concatenate([xyz, rgb], 1), 3, None, False), xyz)
    p = prepare_cloud(xyz, 6, [0.1, 0.2, 0.3], False)
    assert p.shape == (50, 6) and np.array_equal(p[:, :3], xyz) and np.allclose(p[:, 3:], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="--color"):
        prepare_cloud(xyz, 6, None, False)
    n = prepare_cloud(np.concatenate([xyz, rgb], 1), 6, None, True)
    assert np.allclose(n[:, :3].mean(0), 0, atol=1e-6) and abs(np.sqrt((n[:, :3] ** 2).sum(1)).max() - 1) < 1e-6 and np.array_equal(n[:, 3:], rgb)
    bad = xyz.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        prepare_cloud(bad, 3, None, False)
    with pytest.raises(ValueError, match="expected"):
        prepare_cloud(np.zeros((5, 4), np.float32), 3, None, False)


def test_a_written_embedding_round_trips_through_the_dataset_loader(tmp_path):
    from oakink2_tamf_amd.dataset.interaction_segment import InteractionSegmentData
    from oakink2_tamf_amd.launch.embed_objects import save_embedding

    emb = np.random.default_rng(1).normal(size=(1, 768)).astype(np.float32)
    save_embedding(str(tmp_path / "C12001.pt"), torch.from_numpy(emb)[0])
    holder = types.SimpleNamespace(interaction_object_list=["C12001"], obj_embedding_prefix=str(tmp_path))
    store = InteractionSegmentData.load_object_embedding(holder)
    assert store["C12001"].shape == (768,) and store["C12001"].dtype == np.float32 and np.array_equal(store["C12001"], emb[0])
    with pytest.raises(ValueError, match="non-finite"):
        save_embedding(str(tmp_path / "x.pt"), torch.full((768,), float("nan")))


@pytest.mark.parametrize("case", ["tiny", "mid", "full"])
def test_the_float64_restatement_equals_the_captured_reference(case):
    """tests/pointenc_fixture.restatement is the reference of tests/test_pointenc_edges_gpu.py, so it is held to the reference's own
    float64 output on the fixture's points and groups.  Gate e32 / 1000 of the fixture: both sides are float64 evaluations of the
    same sums, whose reordering noise is about 2^-29 of the float32 noise e32, so this leaves six orders of margin and still puts
    the restatement 4000 x inside the 4 * e32 gate that it carries on the GPU.  Measured: 1.7e-15 (tiny), 2.6e-15 (mid), 2.2e-15
    (full, 1.3 s) against e32 of 1.0e-6, 1.6e-6, 1.4e-6."""
    fix = load_golden(f"pointenc_{case}.npz")
    cfg = F.CASES[case][0]
    sd = F.seeded_state_dict(cfg, int(fix["weight_seed"]))
    assert F.state_checksum(sd) == str(fix["state_checksum"]), "the seeded weights are not the ones the fixture was captured with"
    got = F.restatement(sd, cfg, fix["points"], fix["centre_idx"], fix["nbr_sorted"], dtype=torch.float64).numpy()
    assert got.shape == fix["out64"].shape and got.dtype == np.float64
    err, e32 = float(np.abs(got - fix["out64"]).max()), float(fix["e32"])
    print(f"{case}: max|restatement - reference| = {err:.3e}, e32 = {e32:.3e}")
    assert e32 > 0 and err <= e32 / 1000


@pytest.mark.parametrize("name", list(F.SWEEP))
def test_every_sweep_case_builds_and_has_a_float32_noise_floor(name):
    from oakink2_tamf_amd.model.point_encoder import expected_shapes, make_cfg

    cfg, N, B = F.SWEEP[name]
    c = F.sweep_case(name)
    G, M = cfg["num_group"], cfg["group_size"]
    assert {k: v.shape for k, v in c["sd"].items()} == expected_shapes(make_cfg(cfg))
    assert c["points"].shape == (B, N, cfg["point_dims"]) and c["points"].dtype == np.float32
    assert c["centre_idx"].shape == (B, G) and c["nbr_idx"].shape == (B, G, M)
    assert all(len(set(r.tolist())) == G for r in c["centre_idx"]) and np.array_equal(c["nbr_idx"][..., 0], c["centre_idx"])
    assert all(len(set(g.tolist())) == M for b in c["nbr_idx"] for g in b) and 0 <= c["nbr_idx"].min() and c["nbr_idx"].max() < N
    assert c["out64"].shape == (B, 2 * cfg["trans_dim"]) and np.isfinite(c["out64"]).all()
    print(f"{name}: e32 = {c['e32']:.3e}, max|out| = {np.abs(c['out64']).max():.2f}")
    assert 0 < c["e32"] < 1e-4


def test_the_sweep_reaches_the_paths_it_is_there_for():
    """the properties that make each case worth its run (T = num_group + 1; the attention LDS is 64 * pe_att_ts(T) + 64 bytes)"""
    def ts(T):
        return (((T + 3) & ~3) + 31) // 32 * 32 + 4

    T = {k: v[0]["num_group"] + 1 for k, v in F.SWEEP.items()}
    pad = {k: -t % 4 for k, t in T.items()}
    assert (T["low"], T["odd"], T["wideE"]) == (2, 16, 17) and F.SWEEP["low"][0]["group_size"] == F.SWEEP["low"][1]
    assert pad["t24"] == 0 and T["t24"] % 8 == 0 and pad["t23"] == 1 and pad["g1024"] == 3 and {0, 1, 2, 3} <= set(pad.values())
    assert 64 * ts(T["g991"]) + 64 <= 65536 < 64 * ts(T["g992"]) + 64 and T["g1024"] == 1025
    assert {16, 48, 80, 1024} <= {v[0]["encoder_dims"] for v in F.SWEEP.values()}
    assert {9, 33, 63, 64} <= {v[0]["group_size"] for v in F.SWEEP.values()} and F.SWEEP["wideD"][0]["trans_dim"] == 1024
    from oakink2_tamf_amd.model.point_encoder import MAX_CLOUDS_PER_CALL
    assert F.SWEEP["odd"][2] == MAX_CLOUDS_PER_CALL + 1


def test_host_emulations_of_fps_and_grouping():
    """host_fps / host_knn against a float64 greedy selection on a cloud without near-ties, and their tie rules on exact ties"""
    xyz = np.random.default_rng(5).uniform(-1, 1, (300, 3)).astype(np.float32)
    idx, gap = F.host_fps(xyz, 20, 7)
    assert gap >= 1e-5 and idx[0] == 7 and len(set(idx.tolist())) == 20
    x64, d = xyz.astype(np.float64), np.full(300, np.inf)
    for i in range(19):
        d = np.minimum(d, ((x64 - x64[idx[i]]) ** 2).sum(-1))
        assert idx[i + 1] == int(np.argmax(d))
    nbr = F.host_knn(xyz, idx, 9)
    d64 = ((x64[None] - x64[idx][:, None]) ** 2).sum(-1)
    assert np.array_equal(nbr, np.argsort(d64, axis=1, kind="stable")[:, :9]) and np.array_equal(nbr[:, 0], idx)
    # exact ties: four copies of one point and a mirror pair about the start
    tie = np.array([[0, 0, 0], [2, 1, 0.5], [0.25, 0, 0], [-2, -1, -0.5], [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32)
    idx, gap = F.host_fps(tie, 7, 0)
    assert idx.tolist() == [0, 1, 3, 2, 0, 0, 0] and gap == 0.0
    assert F.host_knn(tie, [4, 1], 5).tolist() == [[0, 4, 5, 6, 2], [1, 2, 0, 4, 5]]
    assert F.host_fps(tie[:1], 1, 0)[0].tolist() == [0]
