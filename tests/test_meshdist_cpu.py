"""The point-to-mesh distance without a GPU: the numpy restatement itself (tests/meshdist_restatement.py, the yardstick of the GPU
tests) against closed forms and a dense sampling, the host half of oakink2_tamf_amd/meshdist.py (validity mask, Morton permutation,
process_sdf's numpy lines), the library's description and exports, and the HIP-free host code of the library (layout, packing,
refusals) through a stand-alone program."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")) if p not in sys.path]

import meshdist_cases as C  # noqa: E402
import meshdist_restatement as MR  # noqa: E402
from oakink2_tamf_amd import _lib  # noqa: E402
from oakink2_tamf_amd import meshdist as MD  # noqa: E402

EPS = 2.0 ** -53


# ---- the restatement itself -------------------------------------------------------------------------------------------------------
def test_axis_aligned_box_closed_form():
    """outside: the distance to the box [lo, hi]; inside: the distance to the nearest wall.  Both are a few roundings of numbers no
    larger than the coordinates (|x| < 0.25 here), so 16 eps absolute is generous and far below any wrong answer."""
    v, f = C.fixture_mesh("aabox")
    lo, hi = v.min(0), v.max(0)
    p = C.points_around(v, 3000, 1).astype(np.float64)
    d = MR.mesh_distance(v, f, p)[0]
    inside = ((p > lo) & (p < hi)).all(1)
    out = np.maximum(np.maximum(lo - p, p - hi), 0.0)
    want = np.where(inside, np.minimum(p - lo, hi - p).min(1), np.sqrt((out * out).sum(1)))
    assert inside.sum() > 50 and (~inside).sum() > 1000
    assert np.abs(d - want).max() <= 16 * EPS


def _barycentric(v, f, face, q):
    a, b, c = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    ab, ac, aq = b - a, c - a, q - a
    d00, d01, d11 = (ab * ab).sum(1), (ab * ac).sum(1), (ac * ac).sum(1)
    d20, d21 = (aq * ab).sum(1), (aq * ac).sum(1)
    den = d00 * d11 - d01 * d01
    vv, ww = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
    resid = np.abs(aq - (ab * vv[:, None] + ac * ww[:, None])).max(1)
    return np.stack([1 - vv - ww, vv, ww], axis=1), resid


@pytest.mark.parametrize("name", ["aabox", "rotbox", "bumpy67", "twoparts"])
def test_closest_point_lies_on_its_face_and_nothing_sampled_is_nearer(name):
    v, f = C.bumpy_grid(67) if name == "bumpy67" else C.fixture_mesh(name)
    p = C.points_around(v, 150, 2).astype(np.float64)
    dist, face, q, d2 = MR.mesh_distance(v, f, p)
    bary, resid = _barycentric(v, f, face, q)
    assert (bary >= -1e-12).all() and (bary <= 1 + 1e-12).all() and resid.max() <= 1e-12
    # a dense barycentric sampling of every face: no sample is nearer by more than 1e-12 relative
    n = 12
    w = np.asarray([(i, j, n - i - j) for i in range(n + 1) for j in range(n + 1 - i)], dtype=np.float64) / n
    tri = v[f]  # (F, 3, 3)
    s = np.einsum("kc,fcx->fkx", w, tri).reshape(-1, 3)
    near = ((p[:, None, :] - s[None, :, :]) ** 2).sum(2).min(1)
    assert (near >= d2 * (1 - 1e-12)).all()
    # and the samples come close - some sample lies within one grid step (longest edge / n) of the true closest point - so the
    # restated distance is no overestimate either
    step = np.sqrt(((tri - np.roll(tri, 1, axis=1)) ** 2).sum(2)).max() / n
    assert (np.sqrt(near) <= dist + step).all()


def test_points_on_vertex_edge_and_face_give_zero():
    v, f = C.flat_grid(131)
    pts, kind = C.on_surface_points(v, f)
    d = MR.mesh_distance(v, f, pts.astype(np.float64))[0]
    assert set(kind.tolist()) == {0, 1, 2} and np.array_equal(d, np.zeros_like(d))


def test_tie_rule_picks_the_lowest_original_index():
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 1.0]], dtype=np.float64)
    f = np.asarray([[1, 3, 2], [0, 1, 2], [1, 2, 4]], dtype=np.int32)  # three faces share the edge 1 - 2
    p = np.asarray([[0.5, 0.5, 0.0], [1.0, 0.0, 0.0], [0.25, 0.75, 0.0], [0.5, 0.5, -1.0]])
    dist, face, q, _ = MR.mesh_distance(v, f, p)
    assert np.array_equal(dist, [0, 0, 0, 1]) and np.array_equal(face, [0, 0, 0, 0])
    for order in ([1, 0, 2], [2, 1, 0], [1, 2, 0]):
        assert np.array_equal(MR.mesh_distance(v, f[order], p)[1], [0, 0, 0, 0])
    # an invalid face in front does not take the tie: indices are the ORIGINAL ones
    g = np.concatenate([[[1, 1, 2]], f]).astype(np.int32)
    assert np.array_equal(MR.mesh_distance(v, g, p)[1], [1, 1, 1, 1])
    # a NaN never wins
    dn, fn, _, _ = MR.mesh_distance(v, f, np.asarray([[np.nan, 0.0, 0.0]]))
    assert np.isinf(dn[0]) and fn[0] == -1


def test_regions_all_occur():
    v, f = C.bumpy_grid(67)
    p = C.points_around(v, 400, 3).astype(np.float64)
    k = MR.closest_on_triangles(v[f[:, 0]], v[f[:, 1]], v[f[:, 2]], p)[2]
    assert set(np.unique(k).tolist()) == set(range(7))


# ---- the host half of meshdist.py -------------------------------------------------------------------------------------------------
def test_validity_mask_and_morton_permutation():
    v, f, bad = C.with_invalid_faces(*C.fixture_mesh("twoparts"))
    ok = MD.valid_faces(v, f)
    assert np.array_equal(np.flatnonzero(~ok), bad) and np.array_equal(ok, MR.valid_faces(v, f))
    assert np.array_equal(np.flatnonzero(~MD.in_range_faces(v, f)), bad[2:])
    perm = MD.morton_permutation(v, f)
    assert perm.dtype == np.int32 and np.array_equal(np.sort(perm), np.flatnonzero(ok))
    tri = v[f[perm].astype(np.int64)]
    code = MD.morton_codes(((tri[:, 0] + tri[:, 1]) + tri[:, 2]) / 3.0)
    assert (np.diff(code.astype(np.int64)) >= 0).all()
    same = np.flatnonzero(np.diff(code.astype(np.int64)) == 0)
    assert (perm[same + 1] > perm[same]).all()  # equal codes by ascending index
    # the order makes a tile compact: the tiles' boxes together are far smaller than with the faces as they come
    def boxes(v, f, order):
        t = v[f[order].astype(np.int64)]
        vol = 0.0
        for s in range(0, len(order), MD.TILE):
            c = t[s:s + MD.TILE].reshape(-1, 3)
            vol += float(np.prod(c.max(0) - c.min(0)))
        return vol
    sv, sf = C.fixture_mesh("sphere")
    assert boxes(sv, sf, MD.morton_permutation(sv, sf)) < 0.25 * boxes(sv, sf, np.random.default_rng(0).permutation(len(sf)))
    # the codes: x is the highest bit of a triple
    assert MD.morton_codes(np.asarray([[0, 0, 0], [0, 0, 1.0], [0, 1.0, 0], [1.0, 0, 0]])).tolist() == [0, 0x09249249, 0x12492492, 0x24924924]


def test_mesh_set_host_side_and_refusals():
    v, f, bad = C.with_invalid_faces(*C.fixture_mesh("twoparts"))
    sv, sf = C.fixture_mesh("sphere")
    ms = MD.MeshSet([(v, f), (sv.astype(np.float32), sf)], upload=False)
    assert ms.M == 2 and ms.vert_off.tolist() == [0, len(v), len(v) + len(sv)] and ms.face_off.tolist() == [0, len(f), len(f) + len(sf)]
    assert ms.perm_off.tolist() == [0, len(f) - 4, len(f) - 4 + len(sf)] and not ms.valid[0][bad].any() and ms.valid[1].all()
    keep = MD.in_range_faces(v, f)
    tri = v[f[keep]].reshape(-1, 3)
    assert np.array_equal(ms.scale3[0], 511 / (tri.max(0) - tri.min(0))) and np.array_equal(ms.translate3[0], 0.5 - ms.scale3[0] * tri.min(0))
    with pytest.raises(MD.MeshDistError, match="mesh 0 has no valid face"):
        MD.MeshSet([(v, np.asarray([[0, 0, 1], [2, 3, 10 ** 6]]))], upload=False)
    with pytest.raises(ValueError, match="faces"):
        MD.MeshSet([(v, np.zeros((0, 3), np.int32))], upload=False)
    with pytest.raises(ValueError, match="no mesh"):
        MD.MeshSet([], upload=False)
    with pytest.raises(MD.MeshDistError, match="not uploaded"):
        ms.distance(np.zeros((1, 3), np.float32), [0])


@pytest.mark.parametrize("name", C.FIXTURES)
def test_process_sdf_numpy_lines_equal_lattice_axes(name):
    from conftest import load_golden
    from oakink2_tamf_amd.metrics import siv

    fx = load_golden(f"siv_lattice_{name}.npz")
    R, ratio = min(int(fx["R"]), 24), float(fx["bbox_expand_ratio"])
    ax = siv.lattice_axes(fx["verts"], ratio, R)
    mask = np.zeros(R ** 3, bool)
    mask[[5, 7]] = True
    dist = np.full(R ** 3, 0.25)
    dist[7] = 0.0
    fields, info = MD.sdf_fields(fx["verts"], ax, dist, mask, ratio, R)
    assert tuple(fields) == MD.SDF_FIELDS and len(MD.SDF_FIELDS) == 12
    for key in ("mesh_center", "extent", "extent_expanded", "tick_unit"):
        assert np.array_equal(fields[key], ax[key])
    if R == int(fx["R"]):
        for key in ("mesh_center", "extent", "extent_expanded", "tick_unit"):
            assert np.array_equal(fields[key], fx[key])
        assert np.array_equal(fields["point"][0], fx["point_first"]) and np.array_equal(fields["point"][-1], fx["point_last"])
    assert fields["resolution"] == R and fields["bbox_expand_ratio"] == ratio and fields["bbox"].shape == (8, 3)
    assert np.array_equal(fields["bbox"].mean(0), ax["mesh_center"]) and np.array_equal(fields["bbox_expanded"], fields["bbox_centered_expanded"] + ax["mesh_center"])
    assert np.array_equal(fields["point"], MR.lattice_points(ax["ticks"]) + ax["mesh_center"])
    # the file's interior points are the lattice's: point[sdf > 0] + centre = lattice_points(ticks, centre, idx)
    sdf = fields["sdf"]
    assert sdf[5] == 0.25 and sdf[7] == 0.0 and (np.delete(sdf, [5, 7]) == -0.25).all()
    assert info == {"n_inside": 2, "n_surface_points": 1}
    assert np.array_equal(fields["point"][sdf > 0] + ax["mesh_center"], siv.lattice_points(ax["ticks"], ax["mesh_center"], [5]))


# ---- the library's description ----------------------------------------------------------------------------------------------------
def test_library_description_and_exports():
    lib = _lib.MESHDIST
    assert _lib.OBJECT_DISTANCE == (lib,) and lib.root == "tamf_meshdist.hip" and lib.headers == ("tamf_meshdist.h", "tamf_hip.h")
    assert lib.sources == ["tamf_device.h", "tamf_mesh.h", "tamf_meshdist.h", "tamf_meshdist.hip", "tamf_meshdist_host.h"]
    assert [o.file for o in lib.outputs] == ["libtamf_meshdist.so"] and lib.outputs[0].exports == _lib.MESHDIST_EXPORTS
    assert "-ffp-contract=off" in lib.outputs[0].flags
    header = open(os.path.join(_lib.INCLUDE, "tamf_meshdist.h")).read()
    declared = sorted(set(re.findall(r"\b(tamf_meshdist_\w+)\s*\(", header)))
    assert declared == sorted(_lib.MESHDIST_EXPORTS)
    # a group of its own: disjoint from every other library's exports, and the old groups are what they were
    others = [l for g in (_lib.LIBRARIES, _lib.PREPROCESSING, _lib.TEXT_PREPROCESSING, _lib.TRAINING, _lib.REFINE_TRAINING, _lib.DENOISER_TRAINING,
                          _lib.OPTIMISER, _lib.RENDERING, _lib.OBJECT_PREPROCESSING) for l in g]
    assert len(others) == 12 and lib not in others
    for o in others:
        for out in o.outputs:
            assert not set(out.exports) & set(_lib.MESHDIST_EXPORTS), o.name
    assert _lib.LIBRARIES == (_lib.SAMPLER, _lib.EVAL, _lib.MANO) and _lib.OBJECT_PREPROCESSING == (_lib.SURFACE,) and _lib.RENDERING == (_lib.RENDER,)
    assert len(_lib.EXPORTS) == 27 and len(_lib.EVAL_EXPORTS) == 4
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    path = lib.build()
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("tamf_"))
    assert syms == sorted(_lib.MESHDIST_EXPORTS)


def test_header_constants_are_the_python_side():
    header = open(os.path.join(_lib.INCLUDE, "tamf_meshdist.h")).read()
    assert int(re.search(r"#define TAMF_MESHDIST_TILE (\d+)", header).group(1)) == MD.TILE == C.TILE
    assert float(re.search(r"#define TAMF_MESHDIST_BOX_MARGIN (\S+)", header).group(1)) == 2.0 ** -20


# ---- the library's host code, by itself -------------------------------------------------------------------------------------------
def test_host_packing_program(tmp_path):
    """tools/meshdist_host_check.cpp includes csrc/tamf_meshdist_host.h (no HIP in it) and checks the layout, the padding of the last
    tile, the boxes and every refusal on the CPU.  (Built plainly here; the same program is what a sanitizer build runs.)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    if not (shutil.which(cxx) or os.path.exists(cxx)):
        pytest.fail("no C++ compiler to build the host check with")
    exe = str(tmp_path / "meshdist_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I", _lib.CSRC, "-o", exe, os.path.join(ROOT, "tools", "meshdist_host_check.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
