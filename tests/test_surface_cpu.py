"""tests/surface_restatement.py checked on its own - the GPU gate of the surface sampler leans on it - and the host-side pieces of
oakink2_tamf_amd/surface.py (the object key, the Philox restatement of the package, the thinning draw, the library's description).
CPU only.

Near-boundary samples (surface_restatement.sample's `near`) of every mesh and sample count tests/test_surface_gpu.py uses, with
seed SEED and key KEY, counted by test_no_sample_of_the_gpu_tests_is_near_a_boundary:
    triangle 0, tetrahedron 0, broken_cube 0, icosphere 0, strip_1e-12 0, block-1 0, block 0, block+1 0, 2blocks+1 0
at each of M = 1, 63, 64, 65, 4096 (the excluded set has measure about 2 F^2 2^-52 <= 2e-9, so 0 is the expected outcome); likewise
the 1 024 and 32 768 samples of the point-cloud tests on the icosphere."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")]

import surface_restatement as SR  # noqa: E402
from oakink2_tamf_amd import _lib, surface as S  # noqa: E402
from oracle import mdm_oracle as O  # noqa: E402


def test_weights_points_and_normals_of_the_restatement():
    v, f = SR.icosphere(2)
    r = SR.sample(v, f, 4096, seed=3, key=5)
    w = r["weights"]
    assert (w >= 0).all() and np.abs(w.sum(1) - 1.0).max() <= 2 ** -52
    v64 = v.astype(np.float64)
    tri = v64[f[r["face"]]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert np.abs(((r["point64"] - tri[:, 0]) * n).sum(1)).max() < 1e-16  # in the plane of the picked face (coordinates ~ 0.05)
    assert np.abs(r["normal"].astype(np.float64) - n).max() < 2 ** -23
    assert np.abs(np.linalg.norm(r["normal"].astype(np.float64), axis=1) - 1).max() < 2 ** -22
    # an icosphere's faces point away from its centre
    assert ((r["point64"] - np.array([0.01, -0.02, 0.03])) * n).sum(1).min() > 0


def test_zero_area_and_invalid_faces_are_never_picked():
    v, f = SR.broken_cube()
    r = SR.sample(v, f, 1 << 14, seed=1, key=2)
    dead = np.flatnonzero(r["area"] == 0)
    assert dead.tolist() == [5, 6, 14]
    assert not np.isin(r["face"], dead).any()
    assert set(r["face"].tolist()) == set(range(15)) - set(dead.tolist())
    assert np.all(np.diff(r["cdf"]) >= 0)


def test_pick_share_follows_the_areas():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 1], [0, 3, 1]], np.float32)  # areas 1 and 3
    f = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    n = 1 << 16
    r = SR.sample(v, f, n, seed=11, key=12)
    assert r["area"].tolist() == [1.0, 3.0]
    share = float((r["face"] == 0).mean())
    sigma = (0.25 * 0.75 / n) ** 0.5
    assert abs(share - 0.25) < 4 * sigma


def test_draws_depend_on_the_sample_index_alone():
    a = SR.draws(0, 100, 5, 6)
    b = SR.draws(37, 63, 5, 6)
    for x, y in zip(a, b):
        assert np.array_equal(x[37:], y) and x.min() > 0 and x.max() <= 1
    assert not np.array_equal(SR.draws(0, 100, 5, 7)[0], a[0]) and not np.array_equal(SR.draws(0, 100, 6, 6)[0], a[0])
    hi = SR.draws(2 ** 32 - 2, 4, 5, 6)[0]  # the counter's high word takes over
    assert len(set(hi.tolist())) == 4


def test_no_sample_of_the_gpu_tests_is_near_a_boundary():
    counts = {}
    for name, (v, f) in SR.gpu_meshes().items():
        counts[name] = [int(SR.sample(v, f, m, SR.SEED, SR.KEY)["near"].sum()) for m in SR.SAMPLE_COUNTS]
    print(counts)
    assert all(c == [0] * len(SR.SAMPLE_COUNTS) for c in counts.values()), counts
    v, f = SR.icosphere(3)
    for n, key in ((1024, S.object_key("icosphere")), (32768, S.object_key("icosphere"))):
        assert int(SR.sample(v, f, n, SR.SEED, key)["near"].sum()) == 0


def test_the_meshes_are_what_the_gpu_tests_say():
    m = SR.gpu_meshes()
    assert [m[k][1].shape[0] for k in ("triangle", "tetrahedron", "broken_cube", "icosphere")] == [1, 4, 15, 1280]
    assert [m[k][1].shape[0] for k in ("block-1", "block", "block+1", "2blocks+1")] == [1023, 1024, 1025, 2049]
    a = SR.areas_and_cross(*m["strip_1e-12"])[0]
    assert a.min() < 1.01e-12 and a.min() > 0.99e-12 and abs(a.max() - 1) < 1e-6


def test_package_philox_and_thinning_equal_the_restatement():
    rng = np.random.default_rng(0)
    c = [rng.integers(0, 2 ** 32, 1000, dtype=np.uint64).astype(np.uint32) for _ in range(4)]
    k0, k1 = 0xA4093822, 0x299F31D0
    for x, y in zip(S.philox4x32_10(*c, k0, k1), O.philox4x32_10(*c, k0, k1)):
        assert x.dtype == np.uint32 and np.array_equal(x, y)
    seed, key = 7, S.object_key("scan")
    assert np.array_equal(S.draw_face_uniform(5, 300, seed, key), SR.draws(5, 300, seed, key)[0])
    for n, keep in ((40000, 32768), (33000, 32768), (10, 10), (100, 1)):
        got = S.thin_indices(n, keep, seed, key)
        assert got.shape == (keep,) and len(set(got.tolist())) == keep and got.min() >= 0 and got.max() < n
        assert np.array_equal(got, SR.thin(n, keep, seed, key)), (n, keep)
    with pytest.raises(ValueError):
        S.thin_indices(5, 6)


def test_object_key_is_fnv1a_64():
    assert S.object_key("") == 0xCBF29CE484222325  # the offset basis
    assert S.object_key("a") == 0xAF63DC4C8601EC8C  # the published test vector of FNV-1a 64
    assert S.object_key("foobar") == 0x85944171F73967E8
    assert S.object_key("O02@0015@00001") != S.object_key("O02@0015@00002")


def test_host_refusals_need_no_gpu():
    v, f = SR.cube()
    with pytest.raises(ValueError, match=r"face 1 = \[0, 3, 8\] has an index outside \[0, 8\)"):
        S.sample_surface(v, np.array([[0, 1, 2], [0, 3, 8]]), 4)
    with pytest.raises(ValueError, match="32768"):
        S.sample_point_cloud(v, f, n_points=8192, oversample=5)
    with pytest.raises(ValueError, match="fewer than the 8"):
        S.resample_points(np.zeros((7, 3), np.float32), 8)
    with pytest.raises(ValueError, match="32768"):
        S.resample_points(np.zeros((40000, 3), np.float32), 32769)
    with pytest.raises(ValueError, match="outside"):
        S.sample_surface(v, f, 4, seed=-1)


def test_library_description_and_exports():
    lib = _lib.SURFACE
    assert _lib.OBJECT_PREPROCESSING == (lib,) and lib.root == "tamf_surface.hip" and lib.headers == ("tamf_surface.h", "tamf_hip.h")
    assert lib.sources == ["tamf_device.h", "tamf_surface.h", "tamf_surface.hip"]
    assert [o.file for o in lib.outputs] == ["libtamf_surface.so"] and lib.outputs[0].exports == _lib.SURFACE_EXPORTS
    header = open(os.path.join(_lib.INCLUDE, "tamf_surface.h")).read()
    import re

    declared = sorted(set(re.findall(r"\b(tamf_surface_\w+)\s*\(", header)))
    assert declared == sorted(_lib.SURFACE_EXPORTS)
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    path = lib.build()
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("tamf_"))
    assert syms == sorted(_lib.SURFACE_EXPORTS)
