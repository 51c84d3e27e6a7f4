"""The winding number without a GPU: the numpy restatement of include/tamf_winding.h against closed forms and the analytic sphere,
the library's description and exports, and the stand-alone host check."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import winding_restatement as WR  # noqa: E402
from test_host_mirror import _declared, _nm_tamf  # noqa: E402

from oakink2_tamf_amd import _lib, winding  # noqa: E402


def _w(verts, faces, pts):
    """(w64, truth, gate) at float64 points"""
    return WR.truth_and_gate(verts, faces, np.asarray(pts, dtype=np.float64).reshape(-1, 3))


def test_longdouble_is_wider():
    WR.require_longdouble()


def test_closed_forms():
    v, f = WR.cube()
    centre = [[0.0, 0.0, 0.0]]
    w, wl, gate = _w(v, f, centre)
    assert abs(w[0] - 1.0) <= gate and abs(float(wl[0]) - 1.0) <= gate and WR.inside(w)[0]
    # without its top: the top's two triangles subtend 4 pi / 6 at the centre
    vo, fo = WR.open_cube()
    w, wl, gate = _w(vo, fo, centre)
    assert abs(w[0] - 5.0 / 6.0) <= gate and abs(float(wl[0] - np.longdouble(5) / 6)) <= gate and WR.inside(w)[0]
    assert w[0] == 0.8333333333333337  # (this cube's float64 value, two units in the last place above 5/6: ten terms of pi / 3 each)
    # flipped: -1, still inside
    w, _, gate = _w(v, f[:, ::-1], centre)
    assert abs(w[0] + 1.0) <= gate and WR.inside(w)[0]
    # two copies
    w, _, gate = _w(np.concatenate([v, v]), np.concatenate([f, f + 8]), centre)
    assert abs(w[0] - 2.0) <= gate and WR.inside(w)[0]
    # far away
    w, _, gate = _w(v, f, [[40.0, -30.0, 25.0], [0.0, 0.0, 1.0e3]])
    assert (np.abs(w) < gate).all() and not WR.inside(w).any()


def test_restatement_inputs_at_the_edges():
    v, f = WR.cube()
    w = WR.winding(v, f, np.asarray([[np.nan, 0.0, 0.0], [0.0, 0.0, 0.0]]))
    assert np.isnan(w[0]) and not WR.inside(w)[0] and WR.inside(w)[1]
    # at a vertex every face through it contributes 0; the other six triangles of the cube give 1/8
    w = WR.winding(v, f, v[:1])
    assert np.isfinite(w).all() and abs(w[0] - 0.125) < 1e-15
    # in the plane of a face and inside it: that face contributes +-1/2
    w = WR.winding(v, f, np.asarray([[0.25, 0.125, 0.5]]))
    assert np.isfinite(w).all() and min(abs(w[0] - 1.0), abs(w[0])) < 1e-15
    # the transform is the header's: rows [R | t] on the widened float32 point
    p = np.asarray([[0.5, -0.25, 2.0]], np.float32)
    t = np.arange(12, dtype=np.float64).reshape(3, 4)
    assert np.array_equal(WR.transform(p, t)[0], t[:, :3] @ p[0].astype(np.float64) + t[:, 3])


def test_uv_sphere_with_poles_on_z():
    """the geometry of the README's failing case of the ray-parity test: inside must equal r < r_in outside the band [r_in, 0.05]"""
    v, f = WR.uv_sphere(16, 32, 0.05)
    assert f.shape[0] == 960 and WR.n_valid(v, f) == 960
    pts = WR.lattice_points(WR.sphere_lattice(0.05, 24, 1.2))
    r = np.linalg.norm(pts, axis=1)
    r_in = WR.inscribed_radius(v, f)
    assert 0.0495 < r_in < 0.0496
    band = (r >= r_in) & (r <= 0.05)
    assert band.mean() <= 0.03, band.mean()
    w, wl, gate = WR.truth_and_gate(v, f, pts)
    assert np.array_equal(WR.inside(w)[~band], (r < r_in)[~band])
    assert np.array_equal(WR.inside(wl)[~band], (r < r_in)[~band])
    assert float(np.abs(np.abs(wl) - 0.5).min()) > 0.49  # a closed mesh: every lattice point is near 0 or near 1
    # with the polar cap removed no lattice point is near the threshold either
    wl_open = WR.winding(v, f[32:], pts, np.longdouble)
    margin = float(np.abs(np.abs(wl_open) - 0.5).min())
    print(f"uv sphere: gate {gate:.3e}, band {band.mean():.4f}, open-cap margin {margin:.4f}")
    assert margin > 100 * gate  # (so `inside` of the open sphere is decided on every lattice point, whatever the last bits of w)


def test_degenerate_face_between_its_vertices_is_left_out():
    """a zero-area face whose collinear vertices straddle the query point would add 2 pi by the formula; the valid-face predicate
    leaves it out, so the mesh with it gives the bits of the mesh alone"""
    v, f = WR.cube()
    v2 = np.concatenate([v, [[-0.25, -0.25, -0.25], [0.25, 0.25, 0.25], [0.125, 0.125, 0.125]]])
    f2 = np.concatenate([f[:5], [[8, 9, 10]], f[5:]]).astype(np.int32)
    pts = np.asarray([[0.0, 0.0, 0.0], [0.1875, 0.1875, 0.1875], [0.1, 0.2, -0.3], [3.0, 0.0, 0.0]])
    assert WR.n_valid(v2, f2) == 12
    a, b = WR.winding(v, f, pts), WR.winding(v2, f2, pts)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    # the formula itself gives +-2 pi for that face at the first point (det = 0 exactly, den a negative rounding residue)
    om = WR.omega(v2[[8, 9, 10]][None], pts[:1])
    assert np.allclose(np.abs(om), 2 * np.pi)


def test_chunked_summation_tree():
    """the total is the serial sum of per-chunk serial sums, not one serial sum: the two differ in the last bits on a mesh of more
    than one chunk, and the restatement follows the header"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import meshdist_cases as MC

    v, f = MC.bumpy_grid(2049)
    pts = MC.points_around(v, 64, seed=1).astype(np.float64)
    idx = np.arange(2049)
    om = WR.omega(v[f[idx]], pts)
    tree = np.zeros(64)
    for c0 in (0, 1024, 2048):
        part = np.zeros(64)
        for k in range(c0, min(c0 + 1024, 2049)):
            part = part + om[:, k]
        tree = tree + part
    assert np.array_equal(WR.winding(v, f, pts), tree / WR.FOUR_PI)
    assert winding.CHUNK == WR.CHUNK == 1024 and winding.FOUR_PI == WR.FOUR_PI == 4 * np.pi


def test_library_description_and_exports():
    lib = _lib.WINDING
    assert _lib.OBJECT_SIGN == (lib,) and lib.root == "tamf_winding.hip" and lib.headers == ("tamf_winding.h", "tamf_hip.h")
    assert lib.sources == ["tamf_winding.hip", "tamf_winding_host.h"]
    assert lib.paths == [_lib.WINDING_LIB_PATH] and lib.outputs[0].flags == ("-ffp-contract=off",) and len(lib.kernels) == 4 and not lib.counted_waits
    declared = _declared("tamf_winding.h")
    assert declared == set(_lib.WINDING_EXPORTS) == set(lib.outputs[0].exports) and len(set(_lib.WINDING_EXPORTS)) == 6
    assert all(s.startswith("tamf_winding_") for s in _lib.WINDING_EXPORTS)
    others = [_lib.EXPORTS, _lib.HOOK_EXPORTS, _lib.EVAL_EXPORTS, _lib.MANO_EXPORTS, _lib.POINTENC_EXPORTS, _lib.TEXTENC_EXPORTS, _lib.ENCTRAIN_EXPORTS,
              _lib.CONTACT_EXPORTS, _lib.REFINETRAIN_EXPORTS, _lib.MDMTRAIN_EXPORTS, _lib.OPTIM_EXPORTS, _lib.RENDER_EXPORTS, _lib.SURFACE_EXPORTS,
              _lib.MESHDIST_EXPORTS, _lib.SDFGRID_EXPORTS]
    for o in others:
        assert not set(o) & set(_lib.WINDING_EXPORTS)
    # the old groups and export lists are what they were
    assert len(_lib.EXPORTS) == 27 and _lib.LIBRARIES == (_lib.SAMPLER, _lib.EVAL, _lib.MANO) and _lib.TRAINING == (_lib.ENCTRAIN, _lib.CONTACT)
    assert _lib.OBJECT_DISTANCE == (_lib.MESHDIST,) and _lib.PENETRATION_LOSS == (_lib.SDFGRID,) and _lib.OBJECT_PREPROCESSING == (_lib.SURFACE,)
    assert len(_lib.MESHDIST_EXPORTS) == 6 and len(_lib.SDFGRID_EXPORTS) == 3 and len(_lib.EVAL_EXPORTS) == 4
    lib.build()
    assert _nm_tamf(lib.paths[0]) == set(_lib.WINDING_EXPORTS)
    assert not lib.stale()
    header = open(os.path.join(_lib.INCLUDE, "tamf_winding.h")).read()
    assert f"#define TAMF_WINDING_CHUNK {winding.CHUNK} " in header
    four_pi = re.search(r"#define TAMF_WINDING_FOUR_PI (\S+)", header).group(1)
    assert float(four_pi) == winding.FOUR_PI == 4 * np.pi
    host = open(os.path.join(_lib.CSRC, "tamf_winding_host.h")).read()
    assert f"constexpr int WN_CHUNK = {winding.CHUNK};" in host
    assert winding.ROUTES == {None: 0, "auto": 0, "loop": 1, "spread": 2}
    assert "#define TAMF_WINDING_FORCE_LOOP 1u" in header and "#define TAMF_WINDING_FORCE_SPREAD 2u" in header


def test_python_refusals_without_a_gpu():
    v, f = WR.cube()
    with pytest.raises(winding.WindingError, match="no valid face"):
        winding.WindingSet([(v, np.asarray([[0, 0, 1], [0, 1, 9]], np.int32))], upload=False)
    with pytest.raises(ValueError, match="no mesh"):
        winding.WindingSet([], upload=False)
    s = winding.WindingSet([(v, f), WR.open_cube()], upload=False)
    assert s.M == 2 and s.valid_off.tolist() == [0, 12, 22] and s.valid_idx[1].tolist() == list(range(10))
    with pytest.raises(winding.WindingError, match="not uploaded"):
        s.points(np.zeros((1, 3), np.float32), [0])
    with pytest.raises(winding.WindingError, match="not uploaded"):
        s.lattice(0, np.zeros((2, 3)))
    with pytest.raises(ValueError, match="sign must be"):
        winding.check_sign("pysdf")
    assert winding.check_sign("parity") == "parity" and winding.check_sign("winding") == "winding"


def test_host_check_program(tmp_path):
    """tools/winding_host_check.cpp includes csrc/tamf_winding_host.h (no HIP in it) and checks every refusal, the chunk table and the
    spread-or-loop decision on the CPU.  (Built plainly here; the same program is what a sanitizer build runs.)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    if not (shutil.which(cxx) or os.path.exists(cxx)):
        pytest.fail("no C++ compiler found for the host check")
    exe = str(tmp_path / "winding_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I", _lib.CSRC, "-o", exe, os.path.join(ROOT, "tools", "winding_host_check.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
