"""GPU: tamf_power_spectrum_sum (csrc/tamf_spectrum.h), metrics.psklj / metrics.contact and the two score launchers.

Bounds (none of them comes from the code under test):
  kernel vs float64 restatement (tests/score_restatement.py, np.fft.fft of the float64 cast): 64 x the gap between a direct float64 DFT
      with exact-index twiddles and np.fft.fft on the same inputs, measured in the test on the CPU; floor 1e-13; relative to each
      feature's largest bin.  Measured gaps on the fixtures: t160 1.7e-15, t7 4.4e-16, degenerate 8.4e-16 - so the floor decides there.
  kernel vs reference fixture (float32 FFT of the reference's numpy): 2 x the fixture's own distance from the restatement
      (1.2e-7 .. 2.0e-7 on the spectra).
  Measured on an MI355X: kernel vs restatement 1.7e-15 (sum) / 2.4e-15 (per clip) on t160, below 7e-16 on the other two; kernel vs reference
      1.2e-7 .. 2.0e-7; end-to-end PSKL-J scores 0 and 1.2e-16 relative from the restatement at a measured tolerance of 1.7e-11.
  The issue also says that a clip of len <= 2 has zero acceleration everywhere.  That holds for len = 1; with len = 2 the held tail gives
  a[0] = (x1 - x1) - (x1 - x0) != 0, so len = 2 is held to the restatement like every other length and only len = 1 to exact zeros."""
import ctypes
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import score_restatement as R  # noqa: E402
from test_score_cpu import CASES, IDS, fixture_gaps, load_case  # noqa: E402

pytestmark = pytest.mark.gpu

FLOOR = 1e-13
MAX_T = 512  # PS_MAX_T of csrc/tamf_spectrum.h


def _psd(joints, lens=None, **kw):
    import torch

    from oakink2_tamf_amd.metrics.psklj import power_spectrum_sum

    return power_spectrum_sum(torch.from_numpy(np.ascontiguousarray(joints)).cuda(), lens, **kw)


def _bound(joints, lens, max_clips=None):
    j = joints if max_clips is None else joints[:max_clips]
    l = lens if (lens is None or max_clips is None) else lens[:max_clips]
    gap = R.rel_to_feature_max(R.direct_dft_spectra(j, l).sum(axis=0), R.spectrum_sum(j, l))
    return max(64.0 * gap, FLOOR)


def _raw(x, lens, accumulate, psd_sum, psd_clip=None, N=None, T=None, F=None):
    """the C entry point itself; tensors or None; -> (rc, message)"""
    import torch

    from oakink2_tamf_amd import hip_backend as hb
    from oakink2_tamf_amd.metrics.psklj import _lib

    L = _lib()
    n, t, f = (x.shape if x is not None else (0, 0, 0))
    lp = None if lens is None else np.ascontiguousarray(np.asarray(lens, np.int32))
    rc = L.tamf_power_spectrum_sum(ctypes.c_void_p(x.data_ptr() if x is not None else 0),
                                   lp.ctypes.data_as(ctypes.c_void_p) if lp is not None else ctypes.c_void_p(0),
                                   n if N is None else N, t if T is None else T, f if F is None else F, accumulate,
                                   ctypes.c_void_p(psd_sum.data_ptr() if psd_sum is not None else 0),
                                   ctypes.c_void_p(psd_clip.data_ptr() if psd_clip is not None else 0),
                                   ctypes.c_void_p(hb._stream_ptr(torch.device("cuda", torch.cuda.current_device()))))
    torch.cuda.synchronize()
    return rc, (L.tamf_last_error(None) or b"").decode()


# ---- 4. fixtures --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prefix", CASES, ids=IDS)
def test_fixtures(name, prefix):
    fx = load_case(name, prefix)
    lens = fx["lens"]
    g_spec, _ = fixture_gaps(fx)
    for joints_key, psd_key in (("dataset_joints", "dataset_psd"), ("model_joints", "model_psd")):
        joints = fx[joints_key]
        N, T = joints.shape[:2]
        L = T - 2
        s, clip = _psd(joints, lens, return_clip=True)
        s, clip = s.cpu().numpy(), clip.cpu().numpy()
        assert s.shape == (L, 63) and clip.shape == (N, L, 63) and s.dtype == np.float64
        want, want_clip = R.spectrum_sum(joints, lens).reshape(L, 63), R.clip_spectra(joints, lens).reshape(N, L, 63)
        bound = _bound(joints, lens)
        e_sum = R.rel_to_feature_max(s, want)
        e_clip = max(R.rel_to_feature_max(clip[n], want_clip[n]) for n in range(N))
        e_ref = R.rel_to_feature_max(s, fx[psd_key].astype(np.float64).sum(axis=0).reshape(L, 63))
        print(f"{name} {prefix}{joints_key}: vs restatement sum {e_sum:.3e} clip {e_clip:.3e} (bound {bound:.3e}); vs reference {e_ref:.3e} "
              f"(2 x gap {2 * g_spec:.3e})")
        assert e_sum <= bound and e_clip <= bound
        assert e_ref <= 2 * g_spec
        # per-clip spectra = what a call on that clip alone sums (0 + p)
        for n in range(N):
            np.testing.assert_array_equal(_psd(joints[n:n + 1], lens[n:n + 1]).cpu().numpy(), clip[n])
        # mirrored bins: k and L - k of a real input carry the same power
        for k in range(1, L):
            scale = np.maximum(np.abs(want).max(axis=0), 1e-300)
            assert (np.abs(s[k] - s[L - k]) / scale).max() <= bound
            assert (np.abs(clip[:, k] - clip[:, L - k]) / np.maximum(np.abs(want_clip).max(axis=1), 1e-300)).max() <= bound


def test_fixture_scores_through_pskl_terms():
    from oakink2_tamf_amd.metrics.psklj import pskl_terms

    for (name, prefix), tag in zip(CASES, IDS):
        fx = load_case(name, prefix)
        _, g_score = fixture_gaps(fx)
        d = _psd(fx["dataset_joints"], fx["lens"]).cpu().numpy().reshape(-1, 21, 3)
        m = _psd(fx["model_joints"], fx["lens"]).cpu().numpy().reshape(-1, 21, 3)
        t = pskl_terms(d, m)
        for got, key in ((t["pskl_gt_model"], "pskl_1"), (t["pskl_model_gt"], "pskl_2")):
            want = float(fx[key])
            err = abs(got - want) / abs(want) if want else abs(got)
            print(f"{tag} {key}: {got!r} vs reference {want!r}: {err:.3e} (2 x gap {2 * g_score:.3e})")
            assert err <= 2 * g_score
        if prefix == "same/":
            assert t["pskl_gt_model"] == 0.0 and t["pskl_model_gt"] == 0.0
        if prefix == "const/":
            assert not d.any()


# ---- 5. bits ------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_chunking_or_feature_position():
    import torch

    rng = np.random.default_rng(77)
    N, T, F = 64, 160, 63
    x = rng.normal(size=(N, T, F)).astype(np.float32)
    lens = rng.integers(1, T + 1, size=N)
    a = _psd(x, lens).cpu().numpy()
    np.testing.assert_array_equal(a, _psd(x, lens).cpu().numpy())  # the same call twice
    xd = torch.from_numpy(x).cuda()
    acc = torch.full((T - 2, F), 7.0, device="cuda", dtype=torch.float64)  # accumulate = 0 overwrites whatever is there
    for c in range(4):
        rc, msg = _raw(xd[16 * c: 16 * c + 16].contiguous(), lens[16 * c: 16 * c + 16], int(c > 0), acc)
        assert rc == 0, msg
    np.testing.assert_array_equal(a, acc.cpu().numpy())
    np.testing.assert_array_equal(a, _psd(x, lens, chunk=7).cpu().numpy())
    # accumulate = 1 continues from what psd_sum holds: a + (second pass over the same clips) = the sum over the clips taken twice
    twice = _psd(np.concatenate([x, x]), np.concatenate([lens, lens])).cpu().numpy()
    rc, msg = _raw(xd, lens, 1, acc)
    assert rc == 0, msg
    np.testing.assert_array_equal(twice, acc.cpu().numpy())
    # a feature's bits do not depend on its column (workgroup tile, lane) nor on the other features
    perm = rng.permutation(F)
    np.testing.assert_array_equal(_psd(x[:, :, perm], lens).cpu().numpy(), a[:, perm])
    np.testing.assert_array_equal(_psd(x[:, :, 5:8], lens).cpu().numpy(), a[:, 5:8])


# ---- 6. sweep -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [3, 63])
@pytest.mark.parametrize("T", [3, 4, 5, 7, 64, 159, 160, 161, 196, MAX_T])
def test_sweep_against_restatement(T, F):
    rng = np.random.default_rng(1000 * T + F)
    L = T - 2
    for N in (1, 2, 33, 257):
        x = (rng.normal(size=(N, T, F)) * rng.uniform(0.01, 1.0, size=(1, 1, F))).astype(np.float32)
        mixed = rng.integers(1, T + 1, size=N)
        for tag, lens in (("len=1", np.full(N, 1)), ("len=2", np.full(N, 2)), ("len=T", np.full(N, T)), ("none", None), ("mixed", mixed)):
            got, clip = _psd(x, lens, return_clip=True)
            got, clip = got.cpu().numpy(), clip.cpu().numpy()
            want = R.spectrum_sum(x, lens)
            bound = _bound(x, lens, max_clips=2)
            err = R.rel_to_feature_max(got, want)
            assert err <= bound, (T, F, N, tag, err, bound)
            assert np.abs(clip.sum(axis=0) - want).max() <= 4 * bound * max(np.abs(want).max(), 1e-300)
            if tag == "len=1":  # one held frame: no acceleration at all
                assert not got.any() and not clip.any()
            if tag == "len=T":
                np.testing.assert_array_equal(got, _psd(x, None).cpu().numpy())


def test_rejected_arguments_launch_nothing():
    import torch

    from oakink2_tamf_amd.hip_backend import TamfError

    x = torch.zeros(2, MAX_T + 1, 3, device="cuda")
    sentinel = torch.full((MAX_T, 3), -5.0, device="cuda", dtype=torch.float64)
    for T, needle in ((2, "at least 3 frames"), (MAX_T + 1, f"above the {MAX_T} frames")):
        rc, msg = _raw(x[:, :T].contiguous(), None, 0, sentinel)
        assert rc == -1 and needle in msg, (rc, msg)
        with pytest.raises(TamfError, match=needle):
            _psd(np.zeros((2, T, 3), np.float32))
    xs = x[:, :8].contiguous()
    for kw, lens, needle in ((dict(N=0), None, "bad shape"), (dict(F=0), None, "bad shape"), ({}, [0, 8], "len[0] = 0 outside [1, T]"),
                             ({}, [8, 9], "len[1] = 9 outside [1, T]")):
        rc, msg = _raw(xs, lens, 0, sentinel, **kw)
        assert rc == -1 and needle in msg, (rc, msg)
    for a, s in ((None, sentinel), (xs, None)):
        rc, msg = _raw(a, None, 0, s, N=2, T=8, F=3)
        assert rc == -1 and "null argument" in msg
    assert bool((sentinel == -5.0).all())  # nothing was launched
    with pytest.raises(ValueError):
        _psd(np.zeros((2, 8, 3), np.float32), [8, 9])
    rc, msg = _raw(x[:, :MAX_T].contiguous(), None, 0, sentinel[: MAX_T - 2])  # the largest accepted T
    assert rc == 0, msg


# ---- 7. canaries --------------------------------------------------------------------------------------------------------------
def test_outputs_stay_inside_their_buffers():
    """psd_sum / psd_clip carved out of larger sentinel-filled tensors: the surroundings are untouched (the entry point allocates
    nothing itself, so the hooks library's guard-band allocator has nothing of it to guard)"""
    import torch

    rng = np.random.default_rng(9)
    for (N, T, F) in ((37, 161, 63), (5, 7, 3), (9, 160, 13)):
        L = T - 2
        x = torch.from_numpy(rng.normal(size=(N, T, F)).astype(np.float32)).cuda()
        lens = rng.integers(1, T + 1, size=N)
        pad = 4096
        big_s = torch.full((2 * pad + L * F,), -3.0, device="cuda", dtype=torch.float64)
        big_c = torch.full((2 * pad + N * L * F,), -3.0, device="cuda", dtype=torch.float64)
        rc, msg = _raw(x, lens, 0, big_s[pad: pad + L * F], big_c[pad: pad + N * L * F])
        assert rc == 0, msg
        for big, n in ((big_s, L * F), (big_c, N * L * F)):
            assert bool((big[:pad] == -3.0).all()) and bool((big[pad + n:] == -3.0).all())
            assert bool((big[pad: pad + n] >= 0.0).all())  # every element written (a power is never negative)
        want = R.spectrum_sum(x.cpu().numpy(), lens)
        assert R.rel_to_feature_max(big_s[pad: pad + L * F].cpu().numpy().reshape(L, F), want) <= _bound(x.cpu().numpy(), lens, max_clips=2)


# ---- 8. Contact Ratio ---------------------------------------------------------------------------------------------------------
def ragged_cr_items(seed=31):
    """clips of different T, len and object count; the hand cloud leaves the object over the clip, so frames fall on both sides of
    the 5 mm threshold - and none within 1e-5 of it (checked on the CPU when this was written: the nearest is 3.4e-4 away)"""
    rng = np.random.default_rng(seed)
    items, verts = [], []
    for (T, nobj, ln) in [(24, 1, 24), (24, 2, 17), (24, 2, 5), (16, 1, 16), (16, 2, 9), (24, 1, 1), (24, 2, 24)]:
        P, V = 96, 778
        pc = rng.normal(size=(nobj, P, 3)) * 0.03
        rot6d = rng.normal(size=(nobj, T, 6))
        tsl = rng.normal(size=(nobj, T, 3)) * 0.02
        traj = np.concatenate([tsl, rot6d], axis=-1).astype(np.float32)
        gap = np.linspace(0.0, 0.3, T)[:, None, None] * np.array([1.0, 0.3, -0.2])
        v = (rng.normal(size=(T, V, 3)) * 0.03 + gap).astype(np.float32)
        items.append({"len": ln, "obj_traj": traj, "obj_pointcloud": pc.astype(np.float32)})
        verts.append(v)
    return items, verts


def test_contact_distances_ragged_batch():
    from oakink2_tamf_amd.metrics.contact import contact_distances, contact_ratio_of

    items, verts = ragged_cr_items()
    want = R.contact_distances(items, verts)
    assert want.shape == (sum(it["len"] for it in items),)
    assert np.abs(want - 0.005).min() > 1e-5  # condition on the inputs: no frame can flip at the threshold
    assert 0.2 < np.mean(want < 0.005) < 0.8
    for bs in (64, 2, 1):
        got = contact_distances(items, verts, batch_size=bs, device="cuda:0")
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
        assert contact_ratio_of(got) == float(np.mean(want < 0.005))


# ---- ground truth through MANO ------------------------------------------------------------------------------------------------
def _per_clip_ground_truth(items, device="cpu"):
    """joints and verts one clip at a time, as the reference does (compute_score_cr.py:247-266): the oracle's pose decode on the host,
    the stand-in layer of the clip's hand_side, + tsl - nothing of launch/_score_common.py"""
    import torch

    import fake_mano
    from oracle import geometry_oracle as G

    layer = dict(zip(("rh", "lh"), fake_mano.make({}, device)[:2]))
    joints, verts = [], []
    for it in items:
        tsl, quat = G.pose_decode(torch.from_numpy(np.asarray(it["pose_repr"], np.float32)))
        mo = layer[it["hand_side"]](pose_coeffs=quat, betas=torch.from_numpy(np.asarray(it["shape"], np.float32)))
        joints.append((mo.joints + tsl.unsqueeze(1)).numpy())
        verts.append((mo.verts + tsl.unsqueeze(1)).numpy())
    return joints, verts


# float32 tolerance of the MANO pass: tests/test_geometry.py holds the HIP pose decode to 2e-6 abs per quaternion component; the stand-in
# layer sums 64 of them against weights of sigma 0.02 (4 sigma = 0.08): 64 x 2e-6 x 0.08 = 1e-5.  A swapped layer, a dropped tsl or a
# misplaced clip is off by 0.1 and more.
MANO_ATOL = 1e-5


def _assert_ground_truth(items, joints, verts):
    want_j, want_v = _per_clip_ground_truth(items)
    for i, it in enumerate(items):
        n = int(it["len"])  # the frames both scores read (CR keeps [:len], PSKL-J holds frame len - 1 from there on)
        assert joints[i].shape == want_j[i].shape == (np.asarray(it["pose_repr"]).shape[0], 21, 3) and verts[i].shape == want_v[i].shape
        assert joints[i].dtype == np.float32 and np.isfinite(joints[i]).all() and np.isfinite(verts[i]).all()
        np.testing.assert_allclose(joints[i][:n], want_j[i][:n], rtol=0, atol=MANO_ATOL, err_msg=f"clip {i} ({it['hand_side']}) joints")
        np.testing.assert_allclose(verts[i][:n], want_v[i][:n], rtol=0, atol=MANO_ATOL, err_msg=f"clip {i} ({it['hand_side']}) verts")


@pytest.mark.parametrize("batch_size", [1, 3, 64])
def test_ground_truth_mano_against_per_clip_rebuild(tmp_path, batch_size):
    import torch

    import fake_mano
    from oakink2_tamf_amd.dataset.interaction_segment import InteractionSegmentData, load_cache_dict
    from oakink2_tamf_amd.launch import _score_common as C
    from oracle import fixtures

    paths, _ = fixtures.write_synthetic_dataset(str(tmp_path), n_segments=7, tag="score")
    ds = InteractionSegmentData(obj_embedding_prefix=paths["emb"], obj_pointcloud_prefix=paths["pc"], cache_dict=load_cache_dict(paths["cache"]))
    items = [ds[i] for i in range(len(ds))]
    sides = [it["hand_side"] for it in items]
    assert sides.count("rh") >= 2 and sides.count("lh") >= 2 and sides != sorted(sides)  # both hands, interleaved in dataset order
    # the two stand-in layers must tell the hands apart for a swap to show
    device = torch.device("cuda:0")
    mano = fake_mano.make({}, device)
    joints, verts = C.ground_truth_mano(items, mano, device, batch_size)
    _assert_ground_truth(items, joints, verts)
    swapped = C.ground_truth_mano(items, (mano[1], mano[0]) + tuple(mano[2:]), device, batch_size)[0]
    assert max(np.abs(a[: int(it["len"])] - b[: int(it["len"])]).max() for a, b, it in zip(joints, swapped, items)) > 1e-2
    with pytest.raises(ValueError, match="unexpected hand_side"):
        C.ground_truth_mano([dict(items[0], hand_side="xx")], mano, device, batch_size)


# ---- 5b. more clips than one launch carries -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1025, 2100])
def test_more_clips_than_one_launch_carries(N):
    """one call with N above the 1024 lengths a launch carries in its arguments (PS_LENS): the entry point issues further launches
    that take their own slice of lengths, clips and psd_clip and continue the sums - same bits as any chunking, right values"""
    rng = np.random.default_rng(N)
    T, F = 12, 63
    x = (rng.normal(size=(N, T, F)) * rng.uniform(0.01, 1.0, size=(1, 1, F))).astype(np.float32)
    lens = rng.integers(1, T + 1, size=N)
    lens[1024:] = np.where(np.arange(N - 1024) % 2 == 0, T, lens[1024:])  # clips past the first launch differ in length from those in it
    one, one_clip = _psd(x, lens, chunk=N, return_clip=True)
    one, one_clip = one.cpu().numpy(), one_clip.cpu().numpy()
    for chunk in (1024, 7):
        s, c = _psd(x, lens, chunk=chunk, return_clip=True)
        np.testing.assert_array_equal(one, s.cpu().numpy())
        np.testing.assert_array_equal(one_clip, c.cpu().numpy())
    bound = _bound(x, lens, max_clips=4)
    want_clip = R.clip_spectra(x, lens)
    assert R.rel_to_feature_max(one, want_clip.sum(axis=0)) <= bound
    scale = np.maximum(np.abs(want_clip).max(axis=1, keepdims=True), 1e-300)
    assert (np.abs(one_clip - want_clip) / scale).max() <= bound
    np.testing.assert_array_equal(_psd(x, None, chunk=N).cpu().numpy(), _psd(x, None, chunk=1024).cpu().numpy())  # the NULL-lengths path


# ---- 9. end to end ------------------------------------------------------------------------------------------------------------
def _run(module, argv, cwd):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-m", module] + argv, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r


def test_launchers_end_to_end(tmp_path):
    """G-stage samples (synthetic .npy) -> launch.sample_refine with tests/fake_mano.py (the tree script/sample_refine.sh leaves) ->
    both score launchers as child processes -> their JSON against the restatements on the same files"""
    import torch

    import fake_mano
    from oakink2_tamf_amd.launch import _score_common as C
    from oakink2_tamf_amd.launch import formats
    from oracle import fixtures
    from oracle import mdm_oracle as O

    root = str(tmp_path)
    # (tag "score": with the stand-in MANO the ground truth of this cache has 6 % of its frames in contact and none nearer than 1.4e-4
    # to the 5 mm threshold - checked on the CPU; the default tag has a frame 1.2e-6 from it)
    paths, cache = fixtures.write_synthetic_dataset(root, tag="score")
    split, name = "test", "arch_mdm_l__0399"
    gdir = os.path.join(root, "common", "sample", "main", "sample", split, name)
    os.makedirs(gdir)
    for i in range(5):
        np.save(os.path.join(gdir, f"{i:06d}.npy"), fixtures.synthetic_sample_pose_repr(name, i))
    torch.save(O.det_state_dict(O.ARCH_REFINE, tag="score/r"), os.path.join(root, "r.pt"))
    data_args = ["--data.process_range", f"?(file:./asset/split/{split}.txt)", "--data.cache_dict_filepath",
                 f"common/save_cache_dict/main/cache/{split}.pkl"]
    _run("oakink2_tamf_amd.launch.sample_refine", data_args + ["--debug.model_weight_filepath", "r.pt", "--debug.sample_save_offset",
                                                               f"{split}/{name}", "--commit", "--mano.factory", "fake_mano:make"], root)
    tree = os.path.join("common", "sample_refine", "main", "sample", split, name)
    score_args = data_args + ["--debug.sample_refine_filepath", tree, "--mano.factory", "fake_mano:make", "--batch_size", "3"]
    got = {}
    for module in ("compute_score_cr", "compute_score_psklj"):
        out_json = os.path.join(root, module + ".json")
        extra = ["--save_dir", os.path.join(root, "cr_dist")] if module == "compute_score_cr" else []
        r = _run("oakink2_tamf_amd.launch." + module, score_args + ["--out_json", out_json] + extra, root)
        with open(out_json) as f:
            got[module] = json.load(f)
        for key in ("n_frames", "gt_contact_ratio", "refined_contact_ratio") if module == "compute_score_cr" else ("n_clips", "pskl_gt_model", "pskl_model_gt"):
            assert f"{key} {got[module][key]!r}" in r.stdout

    # the same files through the restatements (the ground-truth MANO pass is the launchers' own call with the launchers' own batching:
    # the stand-in layer's matmul is not what is under test, and its float32 rounding must not differ between the two sides)
    cfg = C.build_config(C.make_parser("x").parse_args(["--data.cache_dict_filepath", paths["cache"], "--data.obj_embedding_prefix", paths["emb"],
                                                        "--data.obj_pointcloud_prefix", paths["pc"], "--debug.sample_refine_filepath",
                                                        os.path.join(root, tree)]))
    pairs = C.load_pairs(cfg)
    infos = cache["interaction_segment_info_list"]
    assert [tuple(p[0]["info"]) for p in pairs] == [tuple(infos[i]) for i in (0, 1, 2, 4)]  # segments 2 and 3 share one info
    items = [p[0] for p in pairs]
    lens = [int(it["len"]) for it in items]
    device = torch.device("cuda:0")
    gt_joints, gt_verts = C.ground_truth_mano(items, fake_mano.make({}, device), device, 3)
    assert {it["hand_side"] for it in items} == {"rh", "lh"}
    _assert_ground_truth(items, gt_joints, gt_verts)  # ... and is itself held to the per-clip rebuild, so the two sides do not share an error
    saved =[formats.read_refine_sample(p[1]) for p in pairs]

    want_gt = R.contact_distances(items, gt_verts)
    want_rf = R.contact_distances(items, [s["verts"] for s in saved])
    assert min(np.abs(want_gt - 0.005).min(), np.abs(want_rf - 0.005).min()) > 1e-5  # (condition of the ragged-batch test)
    cr = got["compute_score_cr"]
    assert cr["n_clips"] == 4 and cr["n_frames"] == sum(lens) == want_gt.shape[0]
    assert cr["gt_contact_ratio"] == float(np.mean(want_gt < 0.005)) and cr["refined_contact_ratio"] == float(np.mean(want_rf < 0.005))
    np.testing.assert_allclose(np.load(os.path.join(root, "cr_dist", "gt_contact_dist.npy")), want_gt, rtol=0, atol=1e-6)
    np.testing.assert_allclose(np.load(os.path.join(root, "cr_dist", "refined_contact_dist.npy")), want_rf, rtol=0, atol=1e-6)

    gj, mj = np.stack(gt_joints), np.stack([np.asarray(s["joints"], np.float32) for s in saved])
    d, m = R.spectrum_sum(gj, lens), R.spectrum_sum(mj, lens)  # (158, 21, 3)
    want = R.pskl(d, m)
    # conditioning of the normalise-and-log step on these inputs: move the restatement's summed spectra by the spectra bound
    # (relative to each feature's largest bin, both signs, either set) and take 10 x the largest relative change of a score
    bd, bm = _bound(gj, lens), _bound(mj, lens)
    sd, sm = bd * np.abs(d).max(axis=0, keepdims=True), bm * np.abs(m).max(axis=0, keepdims=True)
    alt = np.where(np.arange(d.shape[0]) % 2 == 0, 1.0, -1.0)[:, None, None]
    change = 0.0
    for pd in (0.0, 1.0, -1.0, alt, -alt):
        for pm in (0.0, 1.0, -1.0, alt, -alt):
            p = R.pskl(np.maximum(d + pd * sd, 0.0), np.maximum(m + pm * sm, 0.0))
            change = max(change, abs(p[0] - want[0]) / abs(want[0]), abs(p[1] - want[1]) / abs(want[1]))
    tol = 10.0 * change
    ps = got["compute_score_psklj"]
    errs = (abs(ps["pskl_gt_model"] - want[0]) / abs(want[0]), abs(ps["pskl_model_gt"] - want[1]) / abs(want[1]))
    print(f"end to end PSKL-J: {ps['pskl_gt_model']!r} {ps['pskl_model_gt']!r} vs {want!r}: rel err {errs[0]:.3e} {errs[1]:.3e}, tolerance {tol:.3e}")
    assert ps["n_clips"] == 4 and ps["n_freq"] == 158 and ps["n_feat"] == 21
    assert tol > 0 and max(errs) <= tol
