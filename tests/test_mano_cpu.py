"""CPU: the native MANO layer away from the GPU - the float64 restatement against analytic cases that do not depend on it,
close_wrist, ManoArrays' validation, the pickle converter, the C header / export list / source closure of libtamf_mano.so (cross-
compiled here), and the factory string through the launchers up to the point where a device is needed."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import mano_fixture as F  # noqa: E402
import mano_restatement as R  # noqa: E402

from oakink2_tamf_amd import mano as M  # noqa: E402

F64 = torch.float64


def _model(V=778, **over):
    d = F.synthetic_arrays(V)
    d.update(over)
    return M.ManoArrays(**d)


def _identity(N):
    q = torch.zeros(N, 16, 4, dtype=F64)
    q[..., 0] = 1
    return q


def _rot(q):
    return R.quat_to_rotmat(torch.as_tensor(q, dtype=F64))


# ---- the restatement against cases that do not depend on it ---------------------------------------------------------------------
@pytest.mark.parametrize("V", [778, 20])
def test_identity_pose_zero_betas_is_the_template(V):
    a = _model(V)
    m = R.to_torch(a, F64)
    verts, joints, j16 = R.mano_forward(m, _identity(2), torch.zeros(2, 10, dtype=F64), center_idx=None)
    vt = torch.from_numpy(a.v_template)
    assert (verts - vt).abs().max() < 1e-14
    want = torch.from_numpy(a.J_regressor @ a.v_template)
    assert (j16 - want).abs().max() < 1e-14
    # the 21 output joints: chain joints and tip vertices in the documented order
    full = torch.cat([want, vt[a.tip_ids.tolist()]])[a.joint_order.tolist()]
    assert (joints - full).abs().max() < 1e-14


def test_root_rotation_is_rigid_about_the_root_joint():
    a = _model()
    m = R.to_torch(a, F64)
    q = _identity(1)
    q[0, 0] = torch.tensor([0.3, -0.5, 0.7, 0.4], dtype=F64)
    verts, _, j16 = R.mano_forward(m, q, torch.zeros(1, 10, dtype=F64), center_idx=None)
    R0 = _rot([0.3, -0.5, 0.7, 0.4])
    assert (R0 @ R0.T - torch.eye(3, dtype=F64)).abs().max() < 1e-14 and abs(float(torch.det(R0)) - 1) < 1e-14
    vt, J0 = torch.from_numpy(a.v_template), torch.from_numpy(a.J_regressor @ a.v_template)[0]
    want = (vt - J0) @ R0.T + J0
    assert (verts[0] - want).abs().max() < 1e-14
    assert (j16[0, 0] - J0).abs().max() < 1e-14


@pytest.mark.parametrize("j", [0, 1, 2, 3, 5, 9, 13, 15])
def test_rotating_a_joint_moves_its_descendants_only(j):
    V = 778
    rng = np.random.default_rng(4)
    bound = rng.integers(0, 16, size=V)
    a = _model(V, posedirs=np.zeros((V, 3, 135)), weights=np.eye(16)[bound])
    m = R.to_torch(a, F64)
    q = _identity(1)
    q[0, j] = torch.tensor([0.6, 0.1, -0.7, 0.2], dtype=F64)
    betas = torch.from_numpy(rng.normal(size=(1, 10)))
    moved = R.mano_forward(m, q, betas, center_idx=None)[0]
    rest = R.mano_forward(m, _identity(1), betas, center_idx=None)[0]
    desc = set()
    for k in range(16):  # k descends from j (j included) when the walk to the root meets j
        p = k
        while p >= 0 and p != j:
            p = F.PARENTS[p]
        if p == j:
            desc.add(k)
    still = torch.from_numpy(~np.isin(bound, sorted(desc)))
    assert desc and (j != 0 or not still.any())
    assert (moved[0][still] - rest[0][still]).abs().max() < 1e-14 if still.any() else True
    assert (moved[0][~still] - rest[0][~still]).abs().max() > 1e-3  # ... and the descendants do move


def test_centering_shifts_everything_by_the_centre_joint():
    a = _model()
    m = R.to_torch(a, F64)
    q, b = (torch.from_numpy(x) for x in F.random_inputs(3))
    v0, j0, _ = R.mano_forward(m, q, b, center_idx=None)
    v1, j1, _ = R.mano_forward(m, q, b, center_idx=0)
    assert (j1[:, 0]).abs().max() == 0
    assert (v0 - j0[:, :1] - v1).abs().max() < 1e-15 and (j0 - j0[:, :1] - j1).abs().max() < 1e-15
    v9, j9, _ = R.mano_forward(m, q, b, center_idx=8)  # a fingertip slot (joint_order[8] = 17)
    assert a.joint_order[8] >= 16 and (j9[:, 8]).abs().max() == 0 and (v9[:, a.tip_ids[1]]).abs().max() == 0


def test_non_unit_quaternions_are_normalised():
    m = R.to_torch(_model(20), F64)
    q, b = F.random_inputs(4)
    s = np.where(np.arange(16) % 2 == 0, 0.5, 3.0)
    qs, _ = F.random_inputs(4, scale=s)
    v0 = R.mano_forward(m, torch.from_numpy(q), torch.from_numpy(b))[0]
    v1 = R.mano_forward(m, torch.from_numpy(qs), torch.from_numpy(b))[0]
    assert (v0 - v1).abs().max() < 1e-14


# ---- close_wrist ----------------------------------------------------------------------------------------------------------------
def _signed_volume(v, f):
    """about the vertex centroid (the open mesh's figure depends on the origin: the centroid lies inside both test meshes)"""
    v = v - v.mean(axis=0)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def _edge_counts(f):
    d = {}
    for a, b, c in f.tolist():
        for e in ((a, b), (b, c), (c, a)):
            d[e] = d.get(e, 0) + 1
    return d


@pytest.mark.parametrize("V", [778, 20])
@pytest.mark.parametrize("flip", [False, True])
def test_close_wrist_is_watertight_and_keeps_the_orientation(V, flip):
    rings, segs = F.SHAPES[V]
    v, f = F.open_sphere(rings, segs)
    if flip:
        f = f[:, ::-1].copy()
    closed = M.close_wrist(f)
    assert closed.shape == (f.shape[0] + segs - 2, 3) and (closed[: f.shape[0]] == f).all() and closed.max() < V
    d = _edge_counts(closed)
    assert all(n == 1 for n in d.values()) and all((b, a) in d for a, b in d)  # every undirected edge: once in each direction
    vol_open, vol = _signed_volume(v, f), _signed_volume(v, closed)
    assert (vol_open > 0) == (not flip) and np.sign(vol) == np.sign(vol_open)
    cap = closed[f.shape[0]:]
    assert (cap[:, 0] == cap[:, 0].min()).all() and cap[:, 0].min() == 1 + (rings - 1) * segs  # a fan from the loop's lowest vertex


def test_close_wrist_rejects_two_holes_no_hole_and_bad_orientation():
    v, f = F.open_sphere(21, 37)
    with pytest.raises(ValueError, match="more than one loop|not a simple loop"):
        M.close_wrist(f[37:])  # the south fan removed as well: two boundary loops
    with pytest.raises(ValueError, match="no hole"):
        M.close_wrist(M.close_wrist(f))
    g = f.copy()
    g[100] = g[100, ::-1]
    with pytest.raises(ValueError):
        M.close_wrist(g)


# ---- ManoArrays -----------------------------------------------------------------------------------------------------------------
def test_mano_arrays_validation(tmp_path):
    d = F.synthetic_arrays(20)
    a = M.ManoArrays(**d)
    assert a.n_verts == 20 and a.parents[0] == -1 and a.v_template.dtype == np.float64
    assert tuple(M.ManoArrays(**F.synthetic_arrays(778)).tip_ids) == M.DEFAULT_TIP_IDS
    with pytest.raises(ValueError, match="shapedirs"):
        M.ManoArrays(**dict(d, shapedirs=d["shapedirs"][:, :, :9]))
    with pytest.raises(ValueError, match="weights"):
        M.ManoArrays(**dict(d, weights=d["weights"].T))
    for bad in ([-1, 0, 1, 2, 0, 4, 6, 0, 7, 8, 0, 10, 11, 0, 13, 14],  # parents[6] = 6: a loop
                [-1, 0, 1, 2, 0, 4, 5, 0, 9, 8, 0, 10, 11, 0, 13, 14],  # parents[8] = 9: parent above its child
                [-1, -1] + F.PARENTS[2:], [3] + F.PARENTS[1:]):         # two roots; joint 0 not the root
        with pytest.raises(ValueError, match="parents"):
            M.ManoArrays(**dict(d, parents=np.array(bad)))
    vt = d["v_template"].copy()
    vt[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        M.ManoArrays(**dict(d, v_template=vt))
    with pytest.raises(TypeError):
        M.ManoArrays(**dict(d, faces=d["faces"].astype(np.float64)))
    with pytest.raises(ValueError, match="tip_ids"):
        M.ManoArrays(**dict(d, tip_ids=np.array([1, 2, 3, 4, 20])))
    with pytest.raises(ValueError, match="permutation"):
        M.ManoArrays(**dict(d, joint_order=np.zeros(21, np.int64)))
    p = str(tmp_path / "m.npz")
    a.to_npz(p)
    b = M.ManoArrays.from_npz(p)
    for k in M.ManoArrays.FIELDS + ("tip_ids", "joint_order"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    assert b.closed_faces is None


# ---- the converter --------------------------------------------------------------------------------------------------------------
def test_converter_round_trips_a_synthetic_pickle(tmp_path):
    import scipy.sparse

    d = F.synthetic_arrays(778)
    kintree = np.stack([np.array([2**32 - 1] + F.PARENTS[1:], dtype=np.uint32), np.arange(16, dtype=np.uint32)])
    pkl = {"v_template": d["v_template"], "shapedirs": d["shapedirs"], "posedirs": d["posedirs"], "weights": d["weights"],
           "J_regressor": scipy.sparse.csc_matrix(d["J_regressor"]), "kintree_table": kintree, "f": d["faces"].astype(np.uint32),
           "hands_mean": np.zeros(45), "bs_style": "lbs"}
    src, dst = str(tmp_path / "MANO_RIGHT.pkl"), str(tmp_path / "MANO_RIGHT.npz")
    with open(src, "wb") as f:
        pickle.dump(pkl, f, protocol=2)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mano_pkl_to_npz.py"), src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    a = M.ManoArrays.from_npz(dst)
    for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "faces"):
        np.testing.assert_array_equal(getattr(a, k), d[k])
    assert a.parents.tolist() == F.PARENTS
    # a pickle that needs a package the user lacks: the error names it
    with open(src, "wb") as f:
        f.write(b"cno_such_mano_dep_pkg\nThing\n.")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mano_pkl_to_npz.py"), src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "no_such_mano_dep_pkg" in r.stderr


# ---- the library's surface ------------------------------------------------------------------------------------------------------
def test_header_exports_and_source_closure():
    from oakink2_tamf_amd import _lib

    with open(os.path.join(ROOT, "include", "tamf_mano.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert set(re.findall(r"\b(tamf_[a-z0-9_]+)\s*\(", hdr)) == set(_lib.MANO_EXPORTS) and len(set(_lib.MANO_EXPORTS)) == len(_lib.MANO_EXPORTS)
    assert not set(_lib.MANO_EXPORTS) & set(_lib.EXPORTS + _lib.EVAL_EXPORTS + _lib.HOOK_EXPORTS)
    assert not [s for s in _lib.SAMPLER.sources + _lib.EVAL.sources if s.startswith("tamf_mano")]
    assert _lib.MANO.sources == ["tamf_device.h", "tamf_mano.h", "tamf_mano.hip"]
    assert len({lib.stamp_path for lib in _lib.LIBRARIES}) == 3
    assert len({lib.digest() for lib in _lib.LIBRARIES}) == 3
    path = _lib.build_mano()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    syms = {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln}
    assert {s for s in syms if s.startswith("tamf_")} == set(_lib.MANO_EXPORTS)
    lib = _lib.load_mano_lib()
    for s in _lib.MANO_EXPORTS:
        getattr(lib, s)


def test_layer_needs_a_gpu_and_refuses_grad():
    if torch.cuda.is_available():
        layer = M.HipManoLayer(_model(20))
        with pytest.raises(RuntimeError, match="inference only"):
            layer(pose_coeffs=torch.zeros(1, 16, 4, requires_grad=True), betas=torch.zeros(1, 10))
        layer.close()
    else:
        with pytest.raises(Exception, match="no MI355X/HIP device"):
            M.HipManoLayer(_model(20))


# ---- the factory string through the launchers -----------------------------------------------------------------------------------
def test_make_mano_resolves_from_the_factory_string(tmp_path, monkeypatch):
    from oakink2_tamf_amd.launch import _score_common as C
    from oakink2_tamf_amd.launch import sample_refine

    seen = {}

    class Stub:
        def __init__(self, arrays, center_idx=0, device=None):
            seen.setdefault("layers", []).append((arrays.n_verts, center_idx, device))
            self.arrays = arrays

        def get_mano_closed_faces(self):
            return torch.from_numpy(M.close_wrist(self.arrays.faces))

    for name, seed in (("MANO_RIGHT.npz", 0), ("MANO_LEFT.npz", 1)):
        M.ManoArrays(**F.synthetic_arrays(778, seed)).to_npz(str(tmp_path / name))
    cfg = C.build_config(C.make_parser("x").parse_args(["--mano.factory", "oakink2_tamf_amd.mano:make_mano", "--mano.mano_path", str(tmp_path)]))
    monkeypatch.setattr(M, "HipManoLayer", Stub)  # everything up to the device: the string, the import, the files, the closed faces
    rh, lh, crh, clh = sample_refine.load_mano(cfg, "cuda:0")
    assert seen["layers"] == [(778, 0, "cuda:0"), (778, 0, "cuda:0")] and rh is not lh
    assert crh.shape == (len(rh.arrays.faces) + 35, 3) and crh.dtype == np.int64 and clh.shape == crh.shape
    with pytest.raises(SystemExit, match="MANO_RIGHT.npz not found"):
        M.make_mano({"mano_path": str(tmp_path / "nowhere")}, "cuda:0")
    with pytest.raises(SystemExit, match="mano_path"):
        M.make_mano({}, "cuda:0")


@pytest.mark.parametrize("module", ["compute_score_cr", "compute_score_siv"])
def test_dry_run_accepts_the_native_factory(tmp_path, module):
    import test_score_cpu as S

    paths, _, tree = S._synthetic_tree(str(tmp_path))
    r = S._launch(module, S._data_args(paths, tree) + ["--mano.factory", "oakink2_tamf_amd.mano:make_mano", "--mano.mano_path", str(tmp_path),
                                                        "--dry_run"], str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
