"""SegmentEncoder (TAMF_KIND_E, tamf_encode) on the MI355X: the reference's fixtures, the float64 restatement over a shape sweep,
batch invariance and determinism bit for bit, refused shapes and calls, and compute_score_fid end to end."""
import ctypes
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from encoder_restatement import ARCH_ENCODER, encoder_forward, load_encoder_case, seeded_inputs, seeded_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
ENCODER_CASES = sorted(glob.glob(os.path.join(HERE, "golden", "segment_encoder_*.npz")))
ARCH_NAMES = ("input_dim", "obj_input_dim", "hand_shape_dim", "obj_embed_dim", "latent_dim", "ff_size", "num_layers", "num_heads")


def _module(case):
    import torch

    from oakink2_tamf_amd.model.segment_encoder import SegmentEncoder

    m = SegmentEncoder(17, **case["arch"]).to("cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in case["sd"].items()})
    return m


def _batch(inputs, device="cuda:0"):
    import torch

    b = {k: torch.from_numpy(np.ascontiguousarray(inputs[k])).to(device) for k in ("pose_repr", "shape", "obj_embedding", "obj_traj")}
    b["hand_side"] = list(inputs["hand_side"])
    return b


def _context(arch, sd, max_batch, max_frames):
    import torch

    from oakink2_tamf_amd.hip_backend import TamfContext

    ctx = TamfContext(arch, max_batch, max_frames, device="cuda:0", kind="E")
    ctx.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return ctx


def _encode(ctx, inputs, obj_num=None):
    import torch

    enc, act = ctx.encode(torch.from_numpy(inputs["pose_repr"]), torch.from_numpy(inputs["shape"]), inputs["hand_side"],
                          torch.from_numpy(inputs["obj_embedding"]), torch.from_numpy(inputs["obj_traj"]), obj_num=obj_num)
    return enc.cpu().numpy(), act.cpu().numpy()


@pytest.mark.parametrize("path", ENCODER_CASES, ids=os.path.basename)
def test_reference_fixture(path):
    case = load_encoder_case(path)
    m = _module(case)
    out = m(_batch(case["inputs"]))
    enc, act = out["encoding"][0].cpu().numpy(), out["activation"].cpu().numpy()
    assert out["encoding"].shape == (1,) + case["out"]["encoding"].shape
    ref_e, ref_a = case["out"]["encoding"], case["out"]["activation"]
    assert np.isfinite(enc).all() and np.isfinite(act).all()
    assert np.abs(enc - ref_e).max() <= 2e-5, np.abs(enc - ref_e).max()
    assert np.abs(act - ref_a).max() <= 2e-5 * np.abs(ref_a).max(), (np.abs(act - ref_a).max(), np.abs(ref_a).max())
    m.close()


def test_obj_num_reproduces_batches_of_one():
    """tamf_encode with per-clip object counts on the padded batch (a) = the reference's clips one at a time (b)"""
    case = load_encoder_case(os.path.join(HERE, "golden", "segment_encoder_b4_t160.npz"))
    m = _module(case)
    out = m.encode(_batch(case["inputs"]), obj_num=case["inputs"]["obj_num"])
    enc, act = out["encoding"][0].cpu().numpy(), out["activation"].cpu().numpy()
    ref_e, ref_a = case["out"]["encoding_single"], case["out"]["activation_single"]
    assert np.abs(enc - ref_e).max() <= 2e-5
    assert np.abs(act - ref_a).max() <= 2e-5 * np.abs(ref_a).max()
    m.close()


def _check_against_restatement(ctx, sd, arch, inputs, obj_num=None):
    enc, act = _encode(ctx, inputs, obj_num)
    re, ra = encoder_forward(sd, arch, inputs["pose_repr"], inputs["shape"], inputs["hand_side"], inputs["obj_embedding"],
                             inputs["obj_traj"], obj_num=obj_num)
    assert np.abs(enc - re).max() <= 2e-5, np.abs(enc - re).max()
    assert np.abs(act - ra).max() <= 2e-5 * max(1.0, np.abs(ra).max()), np.abs(act - ra).max()


@pytest.mark.parametrize("num_layers", [1, 2, 3])
def test_sweep_frames(num_layers):
    arch = dict(ARCH_ENCODER, num_layers=num_layers)
    sd = seeded_state_dict(arch, seed=100 + num_layers)
    ctx = _context(arch, sd, 3, 224)
    for T in (1, 2, 15, 16, 17, 60, 160, 196, 224):
        inputs = seeded_inputs(3, T, 2, seed=T * 7 + num_layers, arch=arch)
        _check_against_restatement(ctx, sd, arch, inputs)
        _check_against_restatement(ctx, sd, arch, inputs, obj_num=[1, 2, 2])
    ctx.close()


def test_sweep_batch():
    sd = seeded_state_dict(ARCH_ENCODER, seed=200)
    ctx = _context(ARCH_ENCODER, sd, 257, 60)
    for B in (1, 3, 64, 257):
        inputs = seeded_inputs(B, 60, 3, seed=B)
        _check_against_restatement(ctx, sd, ARCH_ENCODER, inputs)
    ctx.close()


@pytest.mark.parametrize("ff_size", [16, 64, 512])
def test_sweep_ff_size(ff_size):
    """every feed-forward width the library accepts is a multiple of 16 in [16, 512]: both ends and one between"""
    arch = dict(ARCH_ENCODER, ff_size=ff_size)
    sd = seeded_state_dict(arch, seed=300 + ff_size)
    ctx = _context(arch, sd, 3, 252)
    for T in (5, 100, 252):  # 252: the longest clip the LDS holds
        _check_against_restatement(ctx, sd, arch, seeded_inputs(3, T, 2, seed=T, arch=arch))
    ctx.close()


def test_batch_invariance_bitwise():
    sd = seeded_state_dict(ARCH_ENCODER, seed=400)
    ctx = _context(ARCH_ENCODER, sd, 64, 160)
    obj_num = [1 + i % 3 for i in range(64)]
    inputs = seeded_inputs(64, 160, 3, seed=401, obj_num=obj_num)
    enc, act = _encode(ctx, inputs, obj_num)
    for i in (0, 1, 17, 63):
        one = {k: (v[i:i + 1] if k != "hand_side" else [v[i]]) for k, v in inputs.items()}
        e1, a1 = _encode(ctx, one, [obj_num[i]])
        assert np.array_equal(e1[0], enc[i]) and np.array_equal(a1[0], act[i]), i
        # and without padding: the clip's own objects only
        own = dict(one, obj_embedding=one["obj_embedding"][:, :obj_num[i]], obj_traj=one["obj_traj"][:, :obj_num[i]])
        e2, _ = _encode(ctx, own, None)
        assert np.array_equal(e2[0], enc[i]), i
    ctx.close()


def test_deterministic_bits():
    sd = seeded_state_dict(ARCH_ENCODER, seed=500)
    ctx = _context(ARCH_ENCODER, sd, 16, 196)
    inputs = seeded_inputs(16, 196, 2, seed=501)
    e1, a1 = _encode(ctx, inputs)
    e2, a2 = _encode(ctx, inputs)
    assert np.array_equal(e1, e2) and np.array_equal(a1, a2)
    ctx.close()


def test_resize_keeps_weights():
    sd = seeded_state_dict(ARCH_ENCODER, seed=600)
    ctx = _context(ARCH_ENCODER, sd, 2, 20)
    ctx.resize(5, 100)
    _check_against_restatement(ctx, sd, ARCH_ENCODER, seeded_inputs(5, 100, 2, seed=601))
    ctx.close()


def test_a_resize_that_runs_out_of_memory_leaves_the_encoder_context_working_at_its_old_size(test_hooks):
    """the E counterpart of the G test of this name in test_hip_guardbands.py: tamf_ctx_resize is one transactional body for every kind.
    With either of an E context's two workspace allocations refused (injected on the host, nothing faults) the call reports it, the
    old workspaces stay - dimensions, guard bands, the same bits from the same call - and a later resize that fits succeeds."""
    import torch

    from oakink2_tamf_amd.hip_backend import TamfError, set_guard_bytes

    sd = seeded_state_dict(ARCH_ENCODER, seed=900)
    inputs = seeded_inputs(2, 8, 2, seed=901)
    args = (torch.from_numpy(inputs["pose_repr"]), torch.from_numpy(inputs["shape"]), inputs["hand_side"],
            torch.from_numpy(inputs["obj_embedding"]), torch.from_numpy(inputs["obj_traj"]))
    set_guard_bytes(4096)  # (every allocation from here on has a guard record: their number tells whether the context's lists are whole)
    try:
        ctx = _context(ARCH_ENCODER, sd, 2, 8)
        ref_e, ref_a = (t.clone() for t in ctx.encode(*args))
        n_guard = ctx.check_guards()
        assert n_guard > 2  # the two workspaces + the weight tables
        for k in (0, 1):  # an E context has exactly two workspace allocations
            assert test_hooks.tamf_test_fail_alloc_after(k) == 0
            try:
                with pytest.raises(TamfError, match=r"keeps its 2 x 8 workspaces.*injected"):
                    ctx.resize(4, 16)
            finally:
                assert test_hooks.tamf_test_fail_alloc_after(-1) == 0
            assert (ctx.max_batch, ctx.max_frames) == (2, 8)
            assert ctx.check_guards() == n_guard
            enc, act = ctx.encode(*args)
            assert torch.equal(enc, ref_e) and torch.equal(act, ref_a), k
        ctx.resize(4, 16)
        _check_against_restatement(ctx, sd, ARCH_ENCODER, seeded_inputs(4, 16, 2, seed=902))
        assert ctx.check_guards() == n_guard
        ctx.close()
    finally:
        set_guard_bytes(0)


@pytest.mark.parametrize("change,max_frames,needle", [
    (dict(latent_dim=128), 100, "latent_dim must be 64"),
    (dict(num_heads=2), 100, "num_heads 4"),
    (dict(ff_size=100), 100, "ff_size must be a multiple of 16"),
    (dict(ff_size=1024), 100, "ff_size must be a multiple of 16"),
    (dict(num_layers=0), 100, "num_layers"),
    ({}, 253, "limit of 252 frames"),
])
def test_rejected_architectures(change, max_frames, needle):
    from oakink2_tamf_amd.hip_backend import TamfContext, TamfError

    with pytest.raises(TamfError, match=needle):
        TamfContext(dict(ARCH_ENCODER, **change), 2, max_frames, device="cuda:0", kind="E")


def test_rejected_precision():
    from oakink2_tamf_amd.hip_backend import TamfContext, TamfError

    with pytest.raises(TamfError, match="fp32 only"):
        TamfContext(ARCH_ENCODER, 2, 16, precision="f16x3", device="cuda:0", kind="E")


def test_generator_calls_on_encoder_context_raise():
    import torch

    from oakink2_tamf_amd.hip_backend import TamfError

    sd = seeded_state_dict(ARCH_ENCODER, seed=700)
    ctx = _context(ARCH_ENCODER, sd, 2, 16)
    with pytest.raises(TamfError, match="SegmentEncoder"):
        ctx.set_cond(None, ["rh", "lh"], torch.zeros(2, 16, 10), torch.zeros(2, 1, 768), torch.zeros(2, 1, 16, 9))
    with pytest.raises(TamfError, match="SegmentEncoder"):
        ctx.set_schedule(np.ones(4), np.ones(4), np.zeros(4))
    x = torch.zeros(2, 99, 1, 16, device="cuda:0")
    for fn, args in ((ctx._L.tamf_denoise, (ctx._h, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(x.data_ptr()), None)),
                     (ctx._L.tamf_refine, (ctx._h, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(x.data_ptr()), None)),
                     (ctx._L.tamf_sample_loop, (ctx._h, None, 0, 0, ctypes.c_void_p(x.data_ptr()), None, 1, None))):
        assert fn(*args) == -2  # TAMF_ERR_STATE
    ctx.close()


def test_encode_on_generator_context_is_state_error():
    import torch

    from oakink2_tamf_amd.hip_backend import TamfContext
    from oracle import mdm_oracle as O

    a = O.ARCH_TINY
    ctx = TamfContext(dict(latent_dim=a.latent_dim, ff_size=a.ff_size, num_layers=a.num_layers, num_heads=a.num_heads), 2, 16,
                      precision="f32", device="cuda:0")
    buf = torch.zeros(4096, device="cuda:0")
    p = ctypes.c_void_p(buf.data_ptr())
    rc = ctx._L.tamf_encode(ctx._h, 1, 4, 1, None, p, p, p, p, p, p, None, None)
    assert rc == -2 and b"SegmentEncoder" in ctx._L.tamf_last_error(ctx._h)
    ctx.close()


def test_compute_score_fid_end_to_end(tmp_path):
    import torch

    from oakink2_tamf_amd.dataset.interaction_segment import InteractionSegmentData, load_cache_dict
    from oakink2_tamf_amd.launch import formats
    from oakink2_tamf_amd.metrics.fid import calculate_activation_statistics, calculate_fid
    from oracle.fixtures import write_synthetic_dataset

    paths, _ = write_synthetic_dataset(str(tmp_path), n_segments=150)
    ds = InteractionSegmentData(obj_embedding_prefix=paths["emb"], obj_pointcloud_prefix=paths["pc"], cache_dict=load_cache_dict(paths["cache"]))
    sd = seeded_state_dict(ARCH_ENCODER, seed=800)
    ckpt = os.path.join(str(tmp_path), "encoder.pth")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, ckpt)
    rng = np.random.default_rng(801)
    gt, gen, seen = [], [], set()
    trees = {"perturbed": os.path.join(str(tmp_path), "srf_perturbed"), "same": os.path.join(str(tmp_path), "srf_same")}
    for i in range(len(ds)):
        it = ds[i]
        if tuple(it["info"]) in seen:
            continue
        seen.add(tuple(it["info"]))
        L = int(it["len"])
        noisy = (it["pose_repr"] + 0.3 * rng.normal(size=it["pose_repr"].shape)).astype(np.float32)  # frames >= len: the launcher zeroes them
        for name, pose in (("perturbed", noisy), ("same", it["pose_repr"])):
            T = pose.shape[0]
            d = formats.build_refine_save_dict(it["info"], it["hand_side"], np.zeros((T, 21, 3)), np.zeros((T, 778, 3)), None,
                                               it["obj_list"], L, it["frame_id"], pose)
            path = formats.refine_sample_path_in(trees[name], it["info"])
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "wb") as f:
                import pickle

                pickle.dump(d, f)
        g = noisy.copy()
        g[L:] = 0.0
        obj_num = [int(it["obj_num"])]
        args = (it["shape"][None], [it["hand_side"]], it["obj_embedding"][None], it["obj_traj"][None])
        gt.append(encoder_forward(sd, ARCH_ENCODER, it["pose_repr"][None], *args, obj_num=obj_num)[0][0])
        gen.append(encoder_forward(sd, ARCH_ENCODER, g[None], *args, obj_num=obj_num)[0][0])
    expected = calculate_fid(calculate_activation_statistics(np.stack(gt)), calculate_activation_statistics(np.stack(gen)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "oakink2-tamf_amd")]))
    got = {}
    for name, tree in trees.items():
        out_json = os.path.join(str(tmp_path), f"fid_{name}.json")
        cmd = [sys.executable, "-m", "oakink2_tamf_amd.launch.compute_score_fid", "--cfg", os.path.join(ROOT, "config", "arch_encoder.yml"),
               "--debug.cache_dict_filepath", paths["cache"], "--data.obj_embedding_prefix", paths["emb"], "--data.obj_pointcloud_prefix",
               paths["pc"], "--debug.sample_refine_filepath", tree, "--debug.encoder_checkpoint_filepath", ckpt, "--batch_size", "16",
               "--out_json", out_json]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        with open(out_json) as f:
            got[name] = json.load(f)
        assert got[name]["n_clips"] == len(gt) and "fid" in r.stdout
    assert abs(got["perturbed"]["fid"] - expected) <= 1e-4 * abs(expected), (got["perturbed"], expected)
    assert abs(got["same"]["fid"]) < 1e-6, got["same"]
