"""CPU: the numpy restatement of include/tamf_sdfgrid.h (tests/sdfgrid_restatement.py) against what it must be - an affine function
comes back, a sphere within the trilinear bound, its gradient is the derivative of its depth, nothing outside the lattice - then the
packing of SDFData fields (sdfgrid.pack_grid / SdfGridSet, device-free), the `pen` term of HandInteractionLoss with the restatement
injected as `pen_fn`, the library's description and the stand-alone program over the host-side argument checks.  The kernels' part,
bit for bit against this restatement, is tests/test_sdfgrid_gpu.py."""
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import fake_mano  # noqa: E402
import sdfgrid_cases as C  # noqa: E402
import sdfgrid_restatement as RS  # noqa: E402
from test_host_mirror import _declared, _nm_tamf  # noqa: E402

from oakink2_tamf_amd import _lib, sdfgrid  # noqa: E402

EPS64 = float(np.finfo(np.float64).eps)
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0], np.float32)


def _one(grid, traj_row, x):
    """restatement of one lattice under one pose at points x (N, 3) float32 -> s, cell, w, pos"""
    R, t = RS.pose(traj_row)
    return RS.sample(grid, R, t, x)


def test_affine_lattice_gives_the_function_back_and_its_gradient_is_a():
    """On the dyadic lattice every value of a . p + b is exact in float32, so the trilinear interpolant IS the function; what remains
    is float64 rounding of the pose, the cell coordinates and the three lerps: a few ulp of the largest value (8 eps64 x 16 allows a
    dozen roundings of numbers below 8)."""
    grid = sdfgrid.pack_grid(C.dyadic_fields())
    assert np.array_equal(grid["values"].astype(np.float64), C.dyadic_fields()["sdf"])  # (exact in float32)
    rng = np.random.default_rng(0)
    tr = C.random_traj(rng, ())
    lo, hi = grid["origin"], grid["origin"] + 4 * grid["step"]
    x = C.world_points(tr, rng.uniform(lo + 1e-3, hi - 1e-3, size=(400, 3)))
    R, t = RS.pose(tr)
    p = RS.object_frame(R, t, x)
    s, cell, w, pos = RS.sample(grid, R, t, x)
    assert pos.all() and (cell >= 0).all()
    want = p @ C.AFFINE_A + C.AFFINE_B
    assert np.max(np.abs(s - want)) <= 128 * EPS64 * 8.0
    assert np.max(np.abs(w - R @ C.AFFINE_A)) <= 1024 * EPS64 * 8.0  # (the differences of neighbouring values are exact, / step too)


def test_sphere_depth_within_the_trilinear_bound():
    """Linear interpolation of f between two nodes h apart errs by at most h^2 / 8 max|f''| along that axis; trilinear interpolation is
    three of them nested, each a convex combination of what the previous stage produced, so the stages' errors add:
    |s - f| <= sum_k h_k^2 / 8 max|d_kk f| over the cell.  For f = r - |p|, d_kk f = -(1 - p_k^2 / |p|^2) / |p|, so |d_kk f| <= 1 / |p|,
    and over the cell |p| >= |p0| - |h| for the query point p0 (the cell's diameter is |h|).  The float32 rounding of the stored values
    adds at most half a float32 ulp of the largest |value| (a convex combination of them)."""
    r, res = 0.3, 24
    ext = np.array([0.9, 0.84, 0.96])
    grid = sdfgrid.pack_grid(C.fields_from(C.sphere_fn(r), [0, 0, 0], ext, res))
    h = grid["step"]
    rng = np.random.default_rng(1)
    d = rng.normal(size=(3000, 3))
    p0 = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(r / 2, r * 0.95, size=(3000, 1))  # (f >= 0.05 r there, above the bound: s stays positive)
    x = p0.astype(np.float32)
    s, _, _, pos = _one(grid, IDENTITY, x)
    pn = np.linalg.norm(x.astype(np.float64), axis=1)
    assert pos.all() and pn.min() >= r / 2 * (1 - 1e-6)
    bound = np.sum(h ** 2) / 8.0 / (pn - np.linalg.norm(h)) + 0.5 * np.spacing(np.float32(np.abs(grid["values"]).max()))
    err = np.abs(s - (r - pn))
    print(f"sphere R = {res}: largest error {err.max():.3e}, its bound {bound[np.argmax(err)]:.3e}, smallest bound {bound.min():.3e}")
    assert (err <= bound).all() and err.max() > 1e-5  # (and the interpolation error is there at all: the bound is not vacuous)


def test_central_differences_of_the_depth_equal_the_gradient():
    """Inside one cell the interpolant is linear in each object coordinate, so under a pose whose rotation is a signed permutation a
    central difference along a world axis is the derivative, up to the rounding of two depths divided by 2 h.  The points sit on the
    2^-16 grid with h = 2^-12, so x +- h is exact in float32; they keep 0.2 of a cell from every cell face and lie where s > 0."""
    grid = sdfgrid.pack_grid(C.fields_from(C.sphere_fn(0.3), [0, 0, 0], [0.9, 0.84, 0.96], 16))
    tr = np.array([0.125, -0.0625, 0.03125, 0, -2.0, 0, 0, 0, 0.5], np.float32)  # rows (0,-1,0), (0,0,1), (-1,0,0)
    R, t = RS.pose(tr)
    assert np.array_equal(R, [[0, -1, 0], [0, 0, 1], [-1, 0, 0]])
    rng = np.random.default_rng(2)
    cells = rng.integers(4, 11, size=(600, 3))
    p = grid["origin"] + (cells + rng.uniform(0.2, 0.8, size=(600, 3))) * grid["step"]
    x = np.round((p @ R.T + t) * 65536.0) / 65536.0
    x = x.astype(np.float32)
    h = np.float32(2.0 ** -12)
    s, cell, w, pos = RS.sample(grid, R, t, x)
    keep = pos & (s > 1e-3)
    assert keep.sum() > 100
    for k in range(3):
        e = np.zeros(3, np.float32)
        e[k] = h
        sp, cp, _, _ = RS.sample(grid, R, t, x + e)
        sm, cm, _, _ = RS.sample(grid, R, t, x - e)
        assert np.array_equal(cp[keep], cell[keep]) and np.array_equal(cm[keep], cell[keep])  # (the same cell)
        fd = (sp - sm) / (2.0 * float(h))
        assert np.max(np.abs(fd - w[:, k])[keep]) <= 64 * EPS64 * 0.3 / float(h)
    assert np.abs(w[keep]).max() > 0.5  # (a sphere's gradient has length about 1)


def test_outside_the_lattice_depth_and_gradient_are_exactly_zero():
    fields = C.dyadic_fields()
    grids = [sdfgrid.pack_grid(fields)]
    lo, hi = grids[0]["origin"], grids[0]["origin"] + 4 * grids[0]["step"]
    eps = np.array([2.0 ** -20, 2.0 ** -20, 2.0 ** -20])
    pts = [lo - eps, hi + eps, [lo[0] - 2.0 ** -20, 0.0, 0.25], [0.5, hi[1] + 2.0 ** -20, 0.25], [100.0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0.25],
           (lo + hi) / 2]
    hand = np.asarray(pts, np.float32).reshape(1, 1, -1, 3)
    traj = IDENTITY.reshape(1, 1, 1, 9)
    depth, cell = RS.forward(grids, hand, traj, [[0]])
    g = RS.backward(grids, hand, traj, [[0]], None, np.ones_like(depth))
    assert np.array_equal(depth[0, 0, 0, :-1], np.zeros(7, np.float32)) and (cell[0, 0, 0, :-1] == -1).all()
    assert np.array_equal(g[0, 0, :-1], np.zeros((7, 3), np.float32)) and not np.signbit(g[0, 0, :-1]).any()
    assert depth[0, 0, 0, -1] > 0 and cell[0, 0, 0, -1] >= 0 and np.array_equal(g[0, 0, -1], C.AFFINE_A.astype(np.float32))
    nan_pose = traj.copy()
    nan_pose[..., 4] = np.nan
    depth, cell = RS.forward(grids, hand, nan_pose, [[0]])
    assert not depth.any() and (cell == -1).all() and not RS.backward(grids, hand, nan_pose, [[0]], None, np.ones_like(depth)).any()
    # a padded object and one without a lattice
    assert not RS.forward(grids, hand, traj, [[-1]])[0].any()
    two = np.concatenate([traj, traj], 1)
    d2, c2 = RS.forward(grids, hand, two, [[0, 0]], [1])
    assert d2[0, 0, 0, -1] > 0 and not d2[0, 1].any() and (c2[0, 1] == -1).all()


def test_the_outer_faces_belong_to_the_lattice_and_u_equal_R_minus_1_to_the_last_cell():
    res = 5
    grid = sdfgrid.pack_grid(C.dyadic_fields(res))
    lo, hi = grid["origin"], grid["origin"] + (res - 1) * grid["step"]
    x = np.asarray([hi, lo, [hi[0], lo[1], hi[2]]], np.float32)
    s, cell, w, pos = _one(grid, IDENTITY, x)
    last = ((res - 2) * res + (res - 2)) * res + (res - 2)
    assert pos.all() and cell.tolist() == [last, 0, (res - 2) * res * res + (res - 2)]
    vals = grid["values"].astype(np.float64)
    assert s.tolist() == [vals[-1], vals[0], vals[((res - 1) * res + 0) * res + (res - 1)]]  # (the node's own value: f = 1 or 0 exactly)
    assert np.array_equal(w, np.broadcast_to(C.AFFINE_A, (3, 3)))


def test_packing_reproduces_the_point_field_and_refuses_what_it_must(tmp_path):
    fields = C.fields_from(C.sphere_fn(0.2, (0.3, 0.1, -0.2)), [0.3, 0.1, -0.2], [0.7, 0.5, 0.9], 9)
    g = sdfgrid.pack_grid(fields)
    last = g["origin"] + 8 * g["step"]
    assert g["res"] == 9 and g["values"].dtype == np.float32 and g["values"].shape == (729,)
    assert np.array_equal(g["values"], fields["sdf"].astype(np.float32))
    assert np.allclose(g["origin"], fields["point"][0], rtol=0, atol=1e-15) and np.allclose(last, fields["point"][-1], rtol=0, atol=1e-15)
    assert np.allclose(g["step"], np.asarray([0.7, 0.5, 0.9]) / 8, rtol=1e-15) and not np.allclose(g["step"], fields["tick_unit"])
    # every node, not only the two ends: point[(i R + j) R + k] = origin + (i, j, k) step
    idx = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(9), indexing="ij"), -1).reshape(-1, 3)
    assert np.allclose(g["origin"] + idx * g["step"], fields["point"], rtol=0, atol=1e-15)

    def bad(**kw):
        return {**fields, **kw}

    for what, broken in (("resolution 1 ", bad(resolution=1)), ("resolution 513", bad(resolution=513)), ("sdf holds", bad(sdf=fields["sdf"][:-1])),
                         ("sdf holds", bad(resolution=8)), ("not positive", bad(extent_expanded=np.array([0.7, 0.0, 0.9]))),
                         ("not positive", bad(extent_expanded=np.array([0.7, -0.5, 0.9]))), ("not positive", bad(extent_expanded=np.array([0.7, np.nan, 0.9]))),
                         ("point field runs", bad(point=fields["point"] + fields["mesh_center"])),  # the centre added twice
                         ("point field runs", bad(point=fields["point"] * (9.0 / 8.0))),
                         ("point field runs", bad(mesh_center=np.zeros(3))), ("point has shape", bad(point=fields["point"][:-1])),
                         ("lack 'sdf'", {k: v for k, v in fields.items() if k != "sdf"})):
        with pytest.raises(ValueError, match=what):
            sdfgrid.pack_grid(broken)
    with pytest.raises(ValueError, match="no grids"):
        sdfgrid.SdfGridSet([], upload=False)

    other = C.dyadic_fields()
    gs = sdfgrid.SdfGridSet([fields, other], upload=False)
    assert gs.G == 2 and gs.grid_off.tolist() == [0, 729, 854] and gs.res.tolist() == [9, 5] and gs.values.shape == (854,)
    assert gs.origin.shape == (2, 3) and gs.step.dtype == np.float64 and np.array_equal(gs.values[729:], other["sdf"].astype(np.float32))
    with pytest.raises(RuntimeError, match="not uploaded"):
        gs.tensors()
    gs.check_ids(torch.tensor([[-1, 0], [1, 1]]))
    for ids in ([[2, 0]], [[-2, 0]]):
        with pytest.raises(ValueError, match="outside"):
            gs.check_ids(torch.tensor(ids))

    # pickles, as script/process_object_sdf.sh writes them
    for name, f in (("mug", fields), ("box", other)):
        with open(tmp_path / f"{name}.pkl", "wb") as fh:
            pickle.dump(dict(f), fh, protocol=4)
    loaded, missing = sdfgrid.SdfGridSet.from_prefix(str(tmp_path), ["box", "ghost", "mug"], upload=False)
    assert missing == ["ghost"] and loaded.index_of == {"box": 0, "mug": 1} and loaded.res.tolist() == [5, 9]
    assert np.array_equal(loaded.values, np.concatenate([gs.values[729:], gs.values[:729]])) and np.array_equal(loaded.origin, gs.origin[::-1])
    assert sdfgrid.SdfGridSet.from_prefix(str(tmp_path), ["ghost"], upload=False) == (None, ["ghost"])
    with open(tmp_path / "broken.pkl", "wb") as fh:
        pickle.dump(bad(resolution=8), fh, protocol=4)
    with pytest.raises(ValueError, match="broken.pkl"):
        sdfgrid.SdfGridSet.from_prefix(str(tmp_path), ["broken"], upload=False)
    table = sdfgrid.grid_ids([["mug"], ["ghost", "box"]], loaded.index_of)
    assert table.dtype == torch.int32 and table.tolist() == [[1, -1], [-1, 0]]


def test_python_side_refusals():
    hv, tr, gid = torch.zeros(2, 3, 5, 3), torch.zeros(2, 4, 3, 9), torch.zeros(2, 4, dtype=torch.int32)
    assert sdfgrid.check_shapes(hv, tr, gid, [4, 1]) == (2, 3, 5, 4, [4, 1])
    for args in ((hv[0], tr, gid, None), (hv, tr[:, :, :2], gid, None), (hv, tr[..., :8], gid, None), (hv, tr, gid[:, :3], None), (hv, tr, gid, [4]),
                 (hv, tr, gid, [4, 5]), (hv, tr, gid, [0, 1])):
        with pytest.raises(ValueError):
            sdfgrid.check_shapes(*args)
    gs = sdfgrid.SdfGridSet([C.dyadic_fields()], upload=False)
    from oakink2_tamf_amd.hip_backend import TamfError

    with pytest.raises(TamfError):  # no CPU path
        sdfgrid.penetration_depth(gs, hv, tr, gid)


# ---------------------------------------------------------------------------------------------------------------- the loss
def _loss_scene(seed=0, B=3, T=4, nobj=2):
    """fake layers, a sphere lattice the fake hand (|verts| around 0.2) lies partly inside, a prediction near the ground truth"""
    rng = np.random.default_rng(seed)
    grids = [sdfgrid.pack_grid(C.fields_from(C.sphere_fn(0.3), [0, 0, 0], [0.9, 0.9, 0.9], 20)),
             sdfgrid.pack_grid(C.fields_from(C.sphere_fn(0.25, (0.05, 0, 0)), [0.05, 0, 0], [0.8, 0.8, 0.8], 12))]
    gt = (rng.normal(size=(B, T, 99)) * 0.5).astype(np.float32)
    gt[..., :3] *= 0.1
    pred = gt + (rng.normal(size=gt.shape) * 0.2).astype(np.float32)
    mask = np.ones((B, T), np.float32)
    mask[1, 2:] = 0
    batch = {"pose_repr": torch.from_numpy(gt), "shape": torch.from_numpy(rng.normal(size=(B, T, 10)).astype(np.float32)), "mask": torch.from_numpy(mask),
             "hand_side": ["rh", "lh", "rh"][:B], "obj_traj": torch.from_numpy(C.random_traj(rng, (B, nobj, T), 0.03)), "obj_num": [2, 1, 2][:B],
             "sdf_grid_id": torch.tensor([[0, 1], [1, 0], [0, -1]][:B], dtype=torch.int32)}
    out = torch.from_numpy(pred).permute(0, 2, 1).unsqueeze(2).contiguous()  # (B, 99, 1, T)
    return grids, out, batch


def _crit(**kw):
    from oakink2_tamf_amd.model.interaction_loss import HandInteractionLoss

    layer_rh, layer_lh = fake_mano.make(None, "cpu")[:2]
    rng = np.random.default_rng(9)
    return HandInteractionLoss(layer_rh, layer_lh, np.stack([rng.permutation(778)[:32], rng.permutation(778)[:32]], 1), rng.uniform(0.5, 1.5, 778).astype(np.float32),
                               1.0, 1.0, 0.1, **kw)


def test_pen_is_absent_and_the_loss_bit_equal_at_coefficient_zero():
    grids, out, batch = _loss_scene()
    loss0, d0 = _crit()(out, {k: v for k, v in batch.items() if k != "sdf_grid_id"})
    loss1, d1 = _crit(coef_pen_loss=0.0, pen_fn=RS.penetration_depth(grids))(out, batch)
    assert list(d0) == list(d1) == ["loss", "rec_joint", "rec_vert", "edge_len", "dist_h", "dist_o"] and "pen" not in d1
    assert loss0.dtype == loss1.dtype == torch.float64 and torch.equal(loss0, loss1)
    assert all(torch.equal(torch.as_tensor(d0[k]), torch.as_tensor(d1[k])) for k in d0)


def test_pen_equals_the_formula_in_float64():
    grids, out, batch = _loss_scene()
    coef = 0.75
    crit = _crit(coef_pen_loss=coef, pen_fn=RS.penetration_depth(grids))
    loss, d = crit(out, batch)
    base, _ = _crit()(out, batch)
    assert list(d)[-1] == "pen" and float(d["pen"]) > 0
    want = 0.0
    T = batch["mask"].shape[1]
    for _, idx, verts_p, _, verts_g, _, mask in crit._per_side(out, batch):
        rows = idx.tolist()
        traj, gid, num = batch["obj_traj"][idx].numpy(), batch["sdf_grid_id"][idx].numpy(), [batch["obj_num"][i] for i in rows]
        dp, _ = RS.forward(grids, verts_p.detach().numpy(), traj, gid, num)
        dg, _ = RS.forward(grids, verts_g.detach().numpy(), traj, gid, num)
        e = np.maximum(dp - dg, np.float32(0)).astype(np.float64) * mask.numpy().astype(np.float64)[:, None, :, None]
        for j in range(len(rows)):
            per_obj = e[j].mean(axis=(-2, -1))  # (nobj,): the padded rows are zero already
            want += T / float(mask[j].sum()) * per_obj[:num[j]].sum() / num[j]
    assert abs(float(d["pen"]) - want) <= 1e-12 * want
    assert abs(float(loss) - (float(base) + coef * want)) <= 1e-12 * abs(float(loss))
    # a prediction equal to the ground truth: the excess is 0 whatever the depth
    same = batch["pose_repr"].permute(0, 2, 1).unsqueeze(2).contiguous()
    assert float(crit(same, batch)[1]["pen"]) == 0.0


def test_refine_terms_pen_is_the_mean_over_the_clips():
    grids, _, batch = _loss_scene()
    rng = np.random.default_rng(4)
    B, T = batch["mask"].shape
    tv = (rng.normal(size=(B, T, 778, 3)) * 0.12).astype(np.float32)
    rv = tv + (rng.normal(size=tv.shape) * 0.03).astype(np.float32)
    out = {"refine_hand_verts": torch.from_numpy(rv), "target_hand_verts": torch.from_numpy(tv), "refine_hand_joints": torch.from_numpy(rv[:, :, :21]),
           "target_hand_joints": torch.from_numpy(tv[:, :, :21])}
    crit = _crit(coef_pen_loss=2.0, pen_fn=RS.penetration_depth(grids))
    loss, d = crit.refine_terms(out, batch)
    base, d0 = _crit().refine_terms(out, batch)
    assert "pen" not in d0 and list(d) == list(d0) + ["pen"]
    gid, num, mask = batch["sdf_grid_id"].numpy(), batch["obj_num"], batch["mask"].numpy().astype(np.float64)
    dp, _ = RS.forward(grids, rv, batch["obj_traj"].numpy(), gid, num)
    dg, _ = RS.forward(grids, tv, batch["obj_traj"].numpy(), gid, num)
    e = np.maximum(dp - dg, np.float32(0)).astype(np.float64) * mask[:, None, :, None]
    per_clip = [T / mask[b].sum() * e[b].mean(axis=(-2, -1))[:num[b]].sum() / num[b] for b in range(B)]
    want = float(np.mean(per_clip))
    assert want > 0 and abs(float(d["pen"]) - want) <= 1e-12 * want and abs(float(loss) - (float(base) + 2.0 * want)) <= 1e-12 * float(loss)


def test_loss_value_errors():
    grids, _, _ = _loss_scene()
    with pytest.raises(ValueError, match="coef_pen_loss"):
        _crit(coef_pen_loss=-1.0, pen_fn=RS.penetration_depth(grids))
    with pytest.raises(ValueError, match="sdf_grids"):
        _crit(coef_pen_loss=1.0)
    _crit(coef_pen_loss=1.0, pen_fn=RS.penetration_depth(grids))
    _crit(coef_pen_loss=1.0, sdf_grids=sdfgrid.SdfGridSet([C.dyadic_fields()], upload=False))  # (bound to the set's penetration_depth)


# ---------------------------------------------------------------------------------------------------------------- the library
def test_library_description_and_exports():
    lib = _lib.SDFGRID
    assert _lib.PENETRATION_LOSS == (lib,) and lib.root == "tamf_sdfgrid.hip" and lib.headers == ("tamf_sdfgrid.h", "tamf_hip.h")
    assert lib.sources == ["tamf_sdfgrid.h", "tamf_sdfgrid.hip", "tamf_sdfgrid_host.h"]
    assert lib.paths == [_lib.SDFGRID_LIB_PATH] and lib.outputs[0].flags == ("-ffp-contract=off",) and len(lib.kernels) == 2 and not lib.counted_waits
    declared = _declared("tamf_sdfgrid.h")
    assert declared == set(_lib.SDFGRID_EXPORTS) == set(lib.outputs[0].exports) and len(set(_lib.SDFGRID_EXPORTS)) == 3
    assert all(s.startswith("tamf_sdfgrid_") for s in _lib.SDFGRID_EXPORTS)
    lib.build()
    assert _nm_tamf(lib.paths[0]) == set(_lib.SDFGRID_EXPORTS)
    assert not lib.stale()
    header = open(os.path.join(_lib.INCLUDE, "tamf_sdfgrid.h")).read()
    assert "#define TAMF_SDFGRID_MIN_RES 2\n" in header and "#define TAMF_SDFGRID_MAX_RES 512\n" in header
    assert (sdfgrid.MIN_RES, sdfgrid.MAX_RES) == (2, 512)


def test_host_check_program(tmp_path):
    """tools/sdfgrid_host_check.cpp includes csrc/tamf_sdfgrid_host.h (no HIP in it) and checks every refusal and the launch geometry
    on the CPU.  (Built plainly here; the same program is what a sanitizer build runs.)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    if not (shutil.which(cxx) or os.path.exists(cxx)):
        pytest.fail("no C++ compiler found for the host check")
    exe = str(tmp_path / "sdfgrid_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I", _lib.CSRC, "-o", exe, os.path.join(ROOT, "tools", "sdfgrid_host_check.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
