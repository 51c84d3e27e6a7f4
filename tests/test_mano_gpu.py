"""GPU: the native MANO layer (libtamf_mano.so, oakink2_tamf_amd.mano.HipManoLayer) against the float64 restatement of the
definition (tests/mano_restatement.py) on synthetic MANO-shaped arrays (tests/mano_fixture.py).

Tolerance: measured, not chosen.  Per case e32 = max |float32 restatement - float64 restatement| on the case's own inputs (the float32
restatement is the arithmetic a torch MANO layer would run; it is not the code under test), and the gate on the HIP output is
4 * e32: both are fp32 sums of the same ~150 + 16 terms in different orders, so their error bounds are of the same order; the factor
covers the ordering difference, not more.  Both sides see the same float32 inputs (the float64 side takes them widened)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import mano_fixture as F  # noqa: E402
import mano_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REF = {}


def _arrays(V, seed=0):
    from oakink2_tamf_amd.mano import ManoArrays

    key = ("arrays", V, seed)
    if key not in _REF:
        _REF[key] = ManoArrays(**F.synthetic_arrays(V, seed))
    return _REF[key]


def _layer(V, seed, center):
    from oakink2_tamf_amd.mano import HipManoLayer

    key = ("layer", V, seed, center)
    if key not in _REF:
        _REF[key] = HipManoLayer(_arrays(V, seed), center_idx=center, device=DEV)
    return _REF[key]


def _inputs(N, seed=0, scale=None):
    q, b = F.random_inputs(N, seed, scale)
    return torch.from_numpy(q).float(), torch.from_numpy(b).float()


def _reference(V, seed, center, q32, b32):
    """(verts64, joints64, e32) of the two restatements on the float32 inputs; computed once per case and left unchanged"""
    key = ("ref", V, seed, center, q32.shape[0], float(q32.double().sum()), float(b32.double().sum()))
    if key not in _REF:
        a = _arrays(V, seed)
        v64, j64, _ = R.mano_forward(R.to_torch(a, torch.float64), q32.double(), b32.double(), center)
        v32, j32, _ = R.mano_forward(R.to_torch(a, torch.float32), q32, b32, center)
        e32 = max(float((v32.double() - v64).abs().max()), float((j32.double() - j64).abs().max()))
        _REF[key] = (v64, j64, e32)
    return _REF[key]


CASES = [(778, N, c, None) for N in (1, 15, 16, 17, 33) for c in (0, None)] + [(20, 17, 0, None), (20, 17, None, None), (778, 17, 8, None),
                                                                               (778, 17, 0, "nonunit")]


@pytest.mark.parametrize("V,N,center,kind", CASES, ids=[f"V{V}-N{N}-c{c}{'-' + k if k else ''}" for V, N, c, k in CASES])
def test_parity_with_the_float64_restatement(V, N, center, kind):
    scale = np.where(np.arange(16) % 2 == 0, 0.5, 3.0) if kind == "nonunit" else None
    q, b = _inputs(N, seed=N, scale=scale)
    v64, j64, e32 = _reference(V, 0, center, q, b)
    layer = _layer(V, 0, center)
    out = layer(pose_coeffs=q.to(DEV), betas=b.to(DEV))
    assert out.verts.shape == (N, V, 3) and out.joints.shape == (N, 21, 3) and out.verts.dtype == torch.float32 and out.verts.is_cuda
    ev = float((out.verts.cpu().double() - v64).abs().max())
    ej = float((out.joints.cpu().double() - j64).abs().max())
    print(f"MANO-PARITY V={V} N={N} center={center} {kind or 'unit'}: e32 {e32:.3e}  hip verts {ev:.3e} joints {ej:.3e}  gate {4 * e32:.3e}")
    assert np.isfinite(ev) and np.isfinite(ej) and e32 > 0
    assert ev <= 4 * e32 and ej <= 4 * e32
    # joints_out NULL: the same vertices, bit for bit
    only = layer.forward(q.to(DEV), b.to(DEV), with_joints=False)
    assert only.joints is None and torch.equal(only.verts, out.verts)
    # the fingertip joints ARE the fingertip vertices
    a = _arrays(V, 0)
    slots = [s for s in range(21) if a.joint_order[s] >= 16]
    tips = [int(a.tip_ids[a.joint_order[s] - 16]) for s in slots]
    assert len(slots) == 5 and torch.equal(out.joints[:, slots], out.verts[:, tips])
    if center is not None:
        assert float(out.joints[:, center].abs().max()) == 0.0


def test_batch_invariance_bit_for_bit():
    """frame k of an N = 33 call = the same frame alone = the same frame elsewhere in a permuted batch; both hands' models alive;
    and no bit depends on the frame tiles per workgroup"""
    q, b = _inputs(33, seed=5)
    q, b = q.to(DEV), b.to(DEV)
    rh, lh = _layer(778, 0, 0), _layer(778, 1, 0)
    perm = torch.from_numpy(np.random.default_rng(0).permutation(33)).to(DEV)
    assert int((perm != torch.arange(33, device=DEV)).sum()) > 25
    outs = {}
    for name, layer in (("rh", rh), ("lh", lh)):
        full = layer(pose_coeffs=q, betas=b)
        outs[name] = full
        shuf = layer(pose_coeffs=q[perm], betas=b[perm])
        assert torch.equal(shuf.verts, full.verts[perm]) and torch.equal(shuf.joints, full.joints[perm])
        for k in (0, 15, 16, 17, 32):
            one = layer(pose_coeffs=q[k: k + 1], betas=b[k: k + 1])
            assert torch.equal(one.verts[0], full.verts[k]) and torch.equal(one.joints[0], full.joints[k]), (name, k)
        for tiles in (1, 2, 4):
            layer.set_tiles(tiles)
            again = layer(pose_coeffs=q, betas=b)
            assert torch.equal(again.verts, full.verts) and torch.equal(again.joints, full.joints), (name, tiles)
        layer.set_tiles(0)
        with pytest.raises(RuntimeError, match="m_tiles"):
            layer.set_tiles(3)
    assert float((outs["rh"].verts - outs["lh"].verts).abs().max()) > 1e-3  # two different models
    again = rh(pose_coeffs=q, betas=b)  # ... and the first is untouched by the second's life
    assert torch.equal(again.verts, outs["rh"].verts)


def test_empty_batch_and_model_lifetime():
    from oakink2_tamf_amd.mano import HipManoLayer

    a = _arrays(20)
    first = HipManoLayer(a, center_idx=0, device=DEV)
    out = first(pose_coeffs=torch.zeros(0, 16, 4, device=DEV), betas=torch.zeros(0, 10, device=DEV))
    assert out.verts.shape == (0, 20, 3) and out.joints.shape == (0, 21, 3)
    q, b = _inputs(3)
    want = first(pose_coeffs=q.to(DEV), betas=b.to(DEV)).verts.clone()
    first.close()
    with pytest.raises(RuntimeError, match="closed"):
        first(pose_coeffs=q.to(DEV), betas=b.to(DEV))
    second = HipManoLayer(a, center_idx=0, device=DEV)
    assert torch.equal(second(pose_coeffs=q.to(DEV), betas=b.to(DEV)).verts, want)
    assert second.th_faces.dtype == torch.int64 and second.th_faces.is_cuda
    cf = second.get_mano_closed_faces()
    assert cf.dtype == torch.int64 and cf.shape == (a.faces.shape[0] + 17, 3)
    with pytest.raises(ValueError, match="betas"):
        second(pose_coeffs=q.to(DEV), betas=b[:2].to(DEV))
    second.close()


def test_segment_refine_model_with_the_native_layer():
    """SegmentRefineModel's whole forward at B = 2, T = 7 with HipManoLayer against the same module given the float32 torch
    restatement as its layers.  h2o_dist is a nearest distance, 1-Lipschitz in the hand vertex, so the gate on the vertices carries
    over: |HIP - f64| <= 4 e32 and |torch f32 - f64| <= e32 give 5 e32 between the two, plus the distance kernel's own rounding
    (8 ulp of the largest distance).  refine_pose_repr: the f32 mode's existing gate (5e-5, tests/test_hip_module.py)."""
    from oakink2_tamf_amd.geometry import pose_repr_to_quat
    from oakink2_tamf_amd.model.segment_refine_model import SegmentRefineModel
    from oracle import mdm_oracle as O

    arch = O.ARCH_TINY_R
    fix = load_golden("refine_tiny_r.npz")
    B, T = 2, 7
    assert fix["x_in"].shape[0] >= B and fix["x_in"].shape[1] >= T
    x_in = torch.from_numpy(fix["x_in"][:B, :T]) * 0.3
    sides = ["rh", "lh"]
    traj = torch.from_numpy(fix["cond/obj_traj"][:B, :, :T])
    nobj = traj.shape[1]
    obj_list = [[f"o{k}" for k in range(nobj)], ["o0"]]
    g = torch.Generator().manual_seed(11)
    clouds = [torch.randn(len(o), 300, 3, generator=g).numpy() * 0.05 for o in obj_list]
    shape = torch.from_numpy(fix["cond/shape"][:B, :T])
    batch = {"sample_pose_repr": x_in.to(DEV), "hand_side": sides, "shape": shape.to(DEV),
             "obj_embedding": torch.from_numpy(fix["cond/obj_embedding"][:B]).to(DEV), "obj_traj": traj.to(DEV), "obj_list": obj_list,
             "obj_pointcloud": clouds}
    sd = O.det_state_dict(arch, tag="tiny_r/w")
    res = {}
    for name, make in (("hip", lambda s: _layer(778, s, 0)), ("torch", lambda s: R.TorchManoLayer(_arrays(778, s), 0, DEV))):
        m = SegmentRefineModel(None, latent_dim=arch.latent_dim, ff_size=arch.ff_size, num_layers=arch.num_layers, num_heads=arch.num_heads,
                               precision="f32", use_pc=True, mano_layer_rh=make(0), mano_layer_lh=make(1))
        m.load_state_dict(sd)
        res[name] = m.to(DEV)(batch)
    # e32 of these inputs (the quaternions the module's own pose decode gives)
    _, quat = pose_repr_to_quat(x_in.to(DEV))
    e32 = max(_reference(778, s, 0, quat[i].cpu(), shape[i])[2] for i, s in enumerate((0, 1)))
    dv = float((res["hip"]["sample_hand_verts"] - res["torch"]["sample_hand_verts"]).abs().max())
    dh = float((res["hip"]["sample_h2o_dist"] - res["torch"]["sample_h2o_dist"]).abs().max())
    dp = float((res["hip"]["refine_pose_repr"] - res["torch"]["refine_pose_repr"]).abs().max())
    gate = 5 * e32 + 8 * float(np.finfo(np.float32).eps) * float(res["torch"]["sample_h2o_dist"].abs().max())
    print(f"MANO-MODULE e32 {e32:.3e}: verts {dv:.3e} h2o_dist {dh:.3e} (gate {gate:.3e}) refine_pose_repr {dp:.3e} (gate 5e-5)")
    assert res["hip"]["sample_hand_verts"].shape == (B, T, 778, 3) and res["hip"]["sample_hand_joints"].shape == (B, T, 21, 3)
    assert res["hip"]["sample_hand_normals"].shape == (B, T, 778, 3)  # th_faces is exposed: the normals kernel ran
    assert dv <= 5 * e32 + 8 * float(np.finfo(np.float32).eps) * float(res["torch"]["sample_hand_verts"].abs().max())
    assert dh <= gate and dp <= 5e-5


def _run(module, argv, cwd):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-m", module] + argv, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r


def test_launchers_with_the_native_factory(tmp_path):
    """launch.sample_refine, then launch.compute_score_cr, with --mano.factory oakink2_tamf_amd.mano:make_mano on a synthetic mano_path
    and nothing third-party: the refine tree holds finite verts / joints of the right shapes and the score launcher reads it"""
    import json

    from oakink2_tamf_amd.launch import formats
    from oakink2_tamf_amd.mano import ManoArrays
    from oracle import fixtures
    from oracle import mdm_oracle as O

    root = str(tmp_path)
    paths, cache = fixtures.write_synthetic_dataset(root, tag="score")
    split, name = "test", "arch_mdm_l__0399"
    gdir = os.path.join(root, "common", "sample", "main", "sample", split, name)
    os.makedirs(gdir)
    for i in range(5):
        np.save(os.path.join(gdir, f"{i:06d}.npy"), fixtures.synthetic_sample_pose_repr(name, i))
    torch.save(O.det_state_dict(O.ARCH_REFINE, tag="score/r"), os.path.join(root, "r.pt"))
    mano_dir = os.path.join(root, "mano")
    os.makedirs(mano_dir)
    for fname, seed in (("MANO_RIGHT.npz", 0), ("MANO_LEFT.npz", 1)):
        ManoArrays(**F.synthetic_arrays(778, seed)).to_npz(os.path.join(mano_dir, fname))
    mano_args = ["--mano.factory", "oakink2_tamf_amd.mano:make_mano", "--mano.mano_path", mano_dir]
    data_args = ["--data.process_range", f"?(file:./asset/split/{split}.txt)", "--data.cache_dict_filepath",
                 f"common/save_cache_dict/main/cache/{split}.pkl"]
    _run("oakink2_tamf_amd.launch.sample_refine", data_args + ["--debug.model_weight_filepath", "r.pt", "--debug.sample_save_offset",
                                                               f"{split}/{name}", "--commit"] + mano_args, root)
    tree = os.path.join("common", "sample_refine", "main", "sample", split, name)
    infos = cache["interaction_segment_info_list"]
    n_faces_closed = F.synthetic_arrays(778)["faces"].shape[0] + 35
    for i in (0, 1, 2, 4):
        d = formats.read_refine_sample(formats.refine_sample_path_in(os.path.join(root, tree), infos[i]))
        T = np.asarray(d["verts"]).shape[0]
        assert np.asarray(d["verts"]).shape == (T, 778, 3) and np.asarray(d["joints"]).shape == (T, 21, 3) and T > 0
        assert np.isfinite(np.asarray(d["verts"])).all() and np.isfinite(np.asarray(d["joints"])).all()
        assert np.asarray(d["faces"]).shape == (n_faces_closed, 3)
    out_json = os.path.join(root, "cr.json")
    _run("oakink2_tamf_amd.launch.compute_score_cr", data_args + ["--debug.sample_refine_filepath", tree, "--batch_size", "3", "--out_json",
                                                                  out_json] + mano_args, root)
    with open(out_json) as f:
        got = json.load(f)
    assert got["n_frames"] > 0 and all(np.isfinite(got[k]) and 0 <= got[k] <= 1 for k in ("gt_contact_ratio", "refined_contact_ratio"))
