"""libtamf_surface.so and oakink2_tamf_amd/surface.py on the GPU against tests/surface_restatement.py (include/tamf_surface.h in numpy
float64): the face picks, points within one float32 ulp of the mesh's largest coordinate, normals, the bit-for-bit properties
(repeat, prefix, split at an odd first_sample, key and seed), the refusals with canary-filled outputs, sample_point_cloud and
resample_points against restatement sampling + the point-encoder tests' host FPS.

Every mesh goes straight to the C entry point (the broken cube's out-of-range index would be refused by sample_surface on the host).
tests/test_surface_cpu.py counts the near-boundary samples of these meshes, seeds and counts: none."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")) if p not in sys.path]

import surface_restatement as SR  # noqa: E402

pytestmark = pytest.mark.gpu

TAMF_ERR_INVALID = -1
MESHES = SR.gpu_meshes()
M_MAX = max(SR.SAMPLE_COUNTS)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the restatement's M_MAX samples of a mesh, computed once and shared (do not modify); a smaller M is its prefix"""
    v, f = MESHES[name]
    return SR.sample(v, f, M_MAX, SR.SEED, SR.KEY)


def _lib():
    from oakink2_tamf_amd import surface as S

    return S._bind()


def c_sample(v, f, M, seed=SR.SEED, key=SR.KEY, first=0, normals=True, faces=True, ws_bytes=None, canary=None, V=None, F=None):
    """tamf_surface_sample on device copies of (v, f): -> (status, points, normals, face index) as numpy (None where not asked for).
    Outputs hold max(M, 1) rows, filled with `canary` first when given."""
    import torch

    from oakink2_tamf_amd.hip_backend import _stream_ptr

    lib, dev = _lib(), torch.device("cuda", torch.cuda.current_device())
    vd, fd = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev)
    rows = max(int(M), 1) if M <= (1 << 20) else 64  # (a count that large is only ever refused)
    fill = 0.0 if canary is None else canary
    pts = torch.full((rows, 3), fill, dtype=torch.float32, device=dev)
    nrm = torch.full((rows, 3), fill, dtype=torch.float32, device=dev) if normals else None
    fi = torch.full((rows,), int(fill), dtype=torch.int32, device=dev) if faces else None
    need = int(lib.tamf_surface_workspace_bytes(f.shape[0]))
    assert need >= 8 * (f.shape[0] + 2)
    ws = torch.zeros(need // 8, dtype=torch.float64, device=dev)
    rc = lib.tamf_surface_sample(vd.data_ptr(), fd.data_ptr(), v.shape[0] if V is None else V, f.shape[0] if F is None else F, int(M), seed, key, first,
                                 pts.data_ptr(), nrm.data_ptr() if normals else None, fi.data_ptr() if faces else None, ws.data_ptr(),
                                 need if ws_bytes is None else ws_bytes, _stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, pts.cpu().numpy(), nrm.cpu().numpy() if normals else None, fi.cpu().numpy() if faces else None


@pytest.mark.parametrize("name", sorted(MESHES))
def test_samples_equal_the_restatement(name):
    v, f = MESHES[name]
    ref = _reference(name)
    vmax = float(np.abs(v).max())
    for M in SR.SAMPLE_COUNTS:
        rc, pts, nrm, fi = c_sample(v, f, M)
        assert rc == 0, _lib().tamf_surface_last_error()
        near = ref["near"][:M]
        assert near.sum() <= 1e-3 * M and near.sum() == 0  # (none with these inputs: tests/test_surface_cpu.py)
        keep = ~near
        assert np.array_equal(fi[keep], ref["face"][:M][keep]), (name, M, int((fi[keep] != ref["face"][:M][keep]).sum()))
        assert ref["area"][fi].min() > 0  # a zero-area face, or one with an index past the vertices, is never picked
        err = np.abs(pts[keep].astype(np.float64) - ref["point64"][:M][keep]).max()
        print(f"{name} M={M}: max |point - float64 restatement| = {err:.3e} (gate {2.0 ** -23 * vmax:.3e}), "
              f"points differing in bits from the rounded restatement: {int((pts[keep] != ref['point'][:M][keep]).any(1).sum())}")
        assert err <= 2.0 ** -23 * vmax
        assert np.abs(nrm[keep].astype(np.float64) - ref["normal"][:M][keep].astype(np.float64)).max() <= 2.0 ** -22
        assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -22


def _bits(*arrays):
    return [a.view(np.uint32) if a.dtype == np.float32 else a for a in arrays]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(*a), _bits(*b)))


@pytest.mark.parametrize("name", ["icosphere", "2blocks+1", "broken_cube"])
def test_bit_for_bit_properties(name):
    v, f = MESHES[name]
    M = 4096
    full = c_sample(v, f, M)[1:]
    assert _same(c_sample(v, f, M)[1:], full)  # the same call twice
    for m in (1, 63, 65, 1000):  # the first m samples do not depend on M
        assert _same(c_sample(v, f, m)[1:], [a[:m] for a in full]), m
    for cut in (1, 63, 2049):  # [0, M) in one call = two calls split at an odd first_sample
        a, b = c_sample(v, f, cut)[1:], c_sample(v, f, M - cut, first=cut)[1:]
        assert _same([np.concatenate([x, y]) for x, y in zip(a, b)], full), cut
    # without the optional outputs the points are the same
    assert np.array_equal(c_sample(v, f, M, normals=False, faces=False)[1].view(np.uint32), full[0].view(np.uint32))
    # samples far along the stream, where the counter's high word is in use
    far = c_sample(v, f, 130, first=2 ** 32 - 65)[1:]
    assert _same([a[65:] for a in far], c_sample(v, f, 65, first=2 ** 32)[1:])
    for kw in (dict(key=SR.KEY + 1), dict(seed=SR.SEED + 1), dict(key=SR.KEY ^ (1 << 40)), dict(seed=SR.SEED ^ (1 << 40))):
        other = c_sample(v, f, M, **kw)[1:]
        assert (other[0] != full[0]).any(1).mean() > 0.99 and (other[2] != full[2]).mean() > 0.5, kw


def test_refusals_leave_the_outputs_untouched():
    lib = _lib()
    v, f = SR.cube()
    canary = 12345.0

    def refused(rc, pts, nrm, fi, word):
        msg = lib.tamf_surface_last_error().decode()
        assert rc == TAMF_ERR_INVALID and word in msg, (rc, msg)
        assert (pts == canary).all() and (nrm == canary).all() and (fi == int(canary)).all()

    flat = np.array([[0, 0, 1], [2, 2, 2], [0, 1, 9], [-1, 2, 3]], np.int32)  # repeated indices and indices outside the vertices
    refused(*c_sample(v, flat, 64, canary=canary), "no face of positive area")
    line = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32)  # three points on a line
    refused(*c_sample(line, np.array([[0, 1, 2]], np.int32), 64, canary=canary), "no face of positive area")
    refused(*c_sample(v, f, 0, canary=canary), "M = 0")
    refused(*c_sample(v, f, 64, canary=canary, F=0), "F = 0")
    refused(*c_sample(v, f, 64, canary=canary, V=0), "V = 0")
    refused(*c_sample(v, f, 64, canary=canary, ws_bytes=8 * 12), "workspace too small")
    refused(*c_sample(v, f, 64, canary=canary, first=-1), "first_sample")
    refused(*c_sample(v, f, 2 ** 31, canary=canary), "M = 2147483648")
    assert lib.tamf_surface_workspace_bytes(0) == TAMF_ERR_INVALID and lib.tamf_surface_workspace_bytes((1 << 26) + 1) == TAMF_ERR_INVALID
    assert lib.tamf_surface_workspace_bytes(1 << 26) >= 8 * ((1 << 26) + (1 << 16) + 1)
    # and a good call still works afterwards
    rc, pts, _, fi = c_sample(v, f, 64, canary=canary)
    assert rc == 0 and (pts != canary).all() and fi.max() < 12


def test_python_wrapper_equals_the_c_entry_point():
    import torch

    from oakink2_tamf_amd import surface as S

    v, f = MESHES["icosphere"]
    pts, nrm, fi = S.sample_surface(v, f, 1000, seed=SR.SEED, key=SR.KEY, first_sample=7, normals=True, faces_out=True)
    assert pts.is_cuda and pts.dtype == torch.float32 and fi.dtype == torch.int64 and nrm.shape == (1000, 3)
    _, p2, n2, f2 = c_sample(v, f, 1000, first=7)
    assert _same([pts.cpu().numpy(), nrm.cpu().numpy(), fi.cpu().numpy()], [p2, n2, f2.astype(np.int64)])
    only = S.sample_surface(torch.from_numpy(v), torch.from_numpy(f).long(), 1000, seed=SR.SEED, key=SR.KEY, first_sample=7)
    assert isinstance(only, torch.Tensor) and torch.equal(only, pts)
    with pytest.raises(S.SurfaceError, match="no face of positive area"):
        S.sample_surface(v, np.array([[0, 0, 1]]), 8)


def _fps_running_minimum(p):
    """the distance of every point of an FPS-ordered cloud to the nearest point before it, in the kernel's float32 expression"""
    p = np.ascontiguousarray(p, np.float32)
    d = np.full(p.shape[0], np.float32(1e10))
    out = []
    for k in range(1, p.shape[0]):
        diff = p - p[k - 1]
        d = np.minimum(d, (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2])
        out.append(d[k])
    return np.asarray(out)


@pytest.mark.parametrize("n_points", [256, 8192])
def test_sample_point_cloud_equals_restated_sampling_and_fps(n_points):
    from oakink2_tamf_amd import surface as S

    v, f = MESHES["icosphere"]
    key = S.object_key("icosphere")
    idx, ref = SR.point_cloud(v, f, n_points, 4, SR.SEED, key)
    assert ref["near"].sum() == 0
    pts, nrm, fi = S.sample_point_cloud(v, f, n_points=n_points, oversample=4, seed=SR.SEED, key=key, normals=True, faces_out=True)
    assert pts.shape == (n_points, 3) and nrm.shape == (n_points, 3) and fi.shape == (n_points,)
    assert np.array_equal(fi.cpu().numpy(), ref["face"][idx])
    assert np.array_equal(pts.cpu().numpy().view(np.uint32), ref["point"][idx].view(np.uint32))  # the kept samples ARE the restated FPS order
    assert np.abs(nrm.cpu().numpy() - ref["normal"][idx]).max() <= 2.0 ** -22
    if n_points == 256:
        d = _fps_running_minimum(pts.cpu().numpy())
        assert np.all(np.diff(d) <= 0) and d[-1] > 0
        with pytest.raises(ValueError, match="32768"):
            S.sample_point_cloud(v, f, n_points=8192, oversample=5)
        alone = S.sample_point_cloud(v, f, n_points=n_points, oversample=4, seed=SR.SEED, key=key)
        assert np.array_equal(alone.cpu().numpy().view(np.uint32), pts.cpu().numpy().view(np.uint32))


def test_resample_points_equals_the_restatement():
    from pointenc_fixture import host_fps

    from oakink2_tamf_amd import surface as S

    rng = np.random.default_rng(5)
    scan = (rng.uniform(-0.1, 0.1, (40000, 3)) * np.array([1.0, 0.6, 1.4])).astype(np.float32)
    key = S.object_key("scan")
    rows = SR.thin(40000, 32768, 9, key)
    want = rows[host_fps(scan[rows], 8192, 0)[0]]
    pts, got = S.resample_points(scan, 8192, seed=9, key=key, indices_out=True)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(pts.cpu().numpy().view(np.uint32), scan[want].view(np.uint32))
    # at or below the FPS kernel's limit the points go straight to FPS, whatever the seed
    small = scan[:3000]
    a, ia = S.resample_points(small, 500, seed=1, key=2, indices_out=True)
    b = S.resample_points(small, 500, seed=3, key=4)
    assert np.array_equal(ia.cpu().numpy(), host_fps(small, 500, 0)[0]) and np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    with pytest.raises(ValueError, match="fewer"):
        S.resample_points(small, 3001)
