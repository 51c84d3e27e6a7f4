"""libtamf_meshdist.so and oakink2_tamf_amd/meshdist.py on the GPU against tests/meshdist_restatement.py (include/tamf_meshdist.h in
numpy float64): dist and face bit for bit, inside byte for byte against geometry.mesh_contains on the restated query points; culling
on and off give the same bits; a job's bits do not depend on the batch it is in; the lattice form equals the points form; the refusals
leave canary-filled outputs alone.  No tolerance anywhere: the definition is exact."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")) if p not in sys.path]

import meshdist_cases as C  # noqa: E402
import meshdist_restatement as MR  # noqa: E402

pytestmark = pytest.mark.gpu

TAMF_ERR_INVALID = -1
T = C.TILE


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name in C.FIXTURES:
        return C.fixture_mesh(name)
    if name.startswith("bumpy"):
        return C.bumpy_grid(int(name[5:]))
    if name.startswith("flat"):
        return C.flat_grid(int(name[4:]))
    if name == "confetti":
        return C.confetti()
    if name == "broken":
        v, f, _ = C.with_invalid_faces(*C.fixture_mesh("twoparts"))
        return v, f
    raise KeyError(name)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def reference(name, kind, n, seed, pose_seed):
    """(query points, dist, face) by the restatement, computed once and shared (do not modify)"""
    v, f = mesh(name)
    q = MR.query_points(points(name, kind, n, seed), pose(pose_seed))
    dist, face, _, _ = MR.mesh_distance(v, f, q)
    return q, dist, face


@functools.lru_cache(maxsize=None)
def points(name, kind, n, seed):
    v, f = mesh(name)
    if kind == "around":
        return C.points_around(v, n, seed)
    if kind == "far":  # far outside every tile box
        return (C.points_around(v, n, seed) + np.float32(1000.0) * np.sign(C.points_around(v, n, seed + 1))).astype(np.float32)
    if kind == "inside_box":  # well inside the mesh's box: inside many tile boxes of the confetti
        return C.points_around(v, n, seed, expand=0.5)
    if kind == "surface":
        return C.on_surface_points(v, f)[0][:n]
    raise KeyError(kind)


def pose(seed):
    return C.IDENTITY if seed is None else C.rigid(seed)


@functools.lru_cache(maxsize=None)
def mesh_set(names):
    from oakink2_tamf_amd.meshdist import MeshSet

    return MeshSet([mesh(n) for n in names])


def inside_reference(name, q):
    import torch

    from oakink2_tamf_amd.geometry import mesh_contains
    from oakink2_tamf_amd.meshdist import in_range_faces

    v, f = mesh(name)
    return mesh_contains(v, f[in_range_faces(v, f)], torch.from_numpy(q).cuda()).cpu().numpy()


def run_jobs(names, jobs, cull=True, inside=True):
    """jobs: [(mesh name, kind, n, seed, pose seed)] -> per job (dist, face, inside) as numpy, one call"""
    pts = [points(j[0], j[1], j[2], j[3]) if j[2] else np.zeros((0, 3), np.float32) for j in jobs]
    ln = np.asarray([len(p) for p in pts], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)
    ms = mesh_set(tuple(names))
    d, f, i = ms.distance(np.concatenate(pts), [names.index(j[0]) for j in jobs], np.stack([pose(j[4]) for j in jobs]), off, ln, inside=inside, cull=cull)
    d, f = d.cpu().numpy(), f.cpu().numpy()
    i = i.cpu().numpy() if inside else None
    o = np.concatenate([[0], np.cumsum(ln)])
    return [(d[o[k]:o[k + 1]], f[o[k]:o[k + 1]], None if i is None else i[o[k]:o[k + 1]]) for k in range(len(jobs))]


def check_job(job, got, inside=True):
    if job[2] == 0:
        assert all(x is None or x.size == 0 for x in got)
        return
    q, dist, face = reference(*job)
    assert np.array_equal(bits(got[0]), bits(dist)), (job, np.flatnonzero(bits(got[0]) != bits(dist))[:5])
    assert np.array_equal(got[1], face), (job, np.flatnonzero(got[1] != face)[:5])
    if inside:
        assert np.array_equal(got[2], inside_reference(job[0], q)), job


# face counts 1, tile - 1, tile, tile + 1, 2 tiles + 3; point counts 1, 63, 64, 65, 778; an empty slice; poses
FACE_CASES = [(f"bumpy{n}", "around", p, 11 + n, ps) for n, p, ps in ((1, 65, None), (T - 1, 64, 1), (T, 63, None), (T + 1, 1, 2), (2 * T + 3, 778, 3))]


@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("job", FACE_CASES, ids=[j[0] for j in FACE_CASES])
def test_face_and_point_counts(job, cull):
    got = run_jobs([job[0]], [job], cull=cull, inside=False)[0]
    check_job(job, got, inside=False)


MIXED_NAMES = ["twoparts", "sphere", "confetti", "broken", "flat131"]
MIXED_JOBS = [
    ("sphere", "around", 778, 21, 4),       # many tiles, a non-identity pose
    ("twoparts", "around", 65, 22, None),
    ("confetti", "inside_box", 256, 23, 5),  # inside many tile boxes at once
    ("broken", "around", 0, 0, None),        # an empty slice
    ("broken", "around", 300, 24, 6),        # invalid faces among valid ones
    ("sphere", "far", 64, 25, None),         # far outside every tile box
    ("flat131", "surface", 607, 0, None),    # on vertices, edges and faces
    ("twoparts", "around", 1, 26, 7),
    ("confetti", "far", 63, 27, 8),
]
SHUFFLED = [MIXED_JOBS[i] for i in (4, 0, 8, 3, 6, 2, 7, 1, 5)]


@pytest.mark.parametrize("cull", [True, False])
def test_mixed_set_matches_the_restatement(cull):
    """two and more meshes of different size in one set, every kind of point, dist / face / inside"""
    for job, got in zip(MIXED_JOBS, run_jobs(MIXED_NAMES, MIXED_JOBS, cull=cull)):
        check_job(job, got)


def test_points_on_the_surface_give_zero():
    job = ("flat131", "surface", 607, 0, None)
    d, f, _ = run_jobs(MIXED_NAMES, [job])[0]
    assert np.array_equal(d, np.zeros_like(d)) and (f >= 0).all()


def test_culling_and_job_order_change_nothing():
    a = run_jobs(MIXED_NAMES, MIXED_JOBS, cull=True)
    b = run_jobs(MIXED_NAMES, MIXED_JOBS, cull=False)
    c = run_jobs(MIXED_NAMES, SHUFFLED, cull=True)
    for k, job in enumerate(MIXED_JOBS):
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), ("cull", job)
        for x, y in zip(a[k], c[SHUFFLED.index(job)]):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), ("order", job)


def test_batch_invariance_alone_and_split():
    job = MIXED_JOBS[0]
    alone = run_jobs(["sphere"], [job])[0]
    among = run_jobs(MIXED_NAMES, MIXED_JOBS)[0]
    for x, y in zip(alone, among):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # the same points split over two calls at an odd place
    ms = mesh_set(("sphere",))
    p = points(*job[:4])
    tr = pose(job[4])[None]
    parts = [ms.distance(p[:301], [0], tr), ms.distance(p[301:], [0], tr)]
    for k in range(3):
        joined = np.concatenate([parts[0][k].cpu().numpy(), parts[1][k].cpu().numpy()])
        assert np.array_equal(joined.view(np.uint8), alone[k].view(np.uint8))


def test_mesh_distance_convenience_and_valid_mask():
    from oakink2_tamf_amd.meshdist import mesh_distance

    v, f = mesh("broken")
    p = points("broken", "around", 300, 24)
    d, fi, ins = mesh_distance(v, f, p)
    q, dist, face = reference("broken", "around", 300, 24, None)
    assert np.array_equal(bits(d.cpu().numpy()), bits(dist)) and np.array_equal(fi.cpu().numpy(), face)
    bad = C.with_invalid_faces(*C.fixture_mesh("twoparts"))[2]
    assert not np.isin(fi.cpu().numpy(), bad).any()
    assert np.array_equal(ins.cpu().numpy(), inside_reference("broken", q))


# ---- lattice ----------------------------------------------------------------------------------------------------------------------
def _ticks(name, R):
    from oakink2_tamf_amd.metrics.siv import lattice_axes

    return lattice_axes(mesh(name)[0], 1.2, R)


LATTICE_CASES = [(n, R) for n in ("rotbox", "aabox") for R in (2, 5, 17, 33)] + [("twoparts", 17), ("torus", 9)]  # (8 x 8 x 4 bricks divide none of them)


@pytest.mark.parametrize("name,R", LATTICE_CASES, ids=[f"{n}-{R}" for n, R in LATTICE_CASES])
def test_lattice_matches_restatement_and_points_form(name, R):
    from oakink2_tamf_amd.meshdist import MeshSet

    ax = _ticks(name, R)
    v, f = ax["verts_centred"], mesh(name)[1]
    ms = MeshSet([(v, f)])
    got = ms.lattice(0, ax["ticks"]).cpu().numpy()
    brute = ms.lattice(0, ax["ticks"], cull=False).cpu().numpy()
    assert got.shape == (R, R, R) and np.array_equal(bits(got), bits(brute))
    q = MR.lattice_points(ax["ticks"])
    want = MR.mesh_distance(v, f, q)[0]
    assert np.array_equal(bits(got.reshape(-1)), bits(want))
    # the points form takes float32 points: the same lattice with its ticks rounded to float32 numbers, identity pose
    t32 = ax["ticks"].astype(np.float32)
    q32 = MR.lattice_points(t32.astype(np.float64))
    lat32 = ms.lattice(0, t32.astype(np.float64)).cpu().numpy().reshape(-1)
    d32 = ms.distance(q32.astype(np.float32), [0], inside=False)[0].cpu().numpy()
    assert np.array_equal(bits(d32), bits(lat32))


def test_process_sdf_sign_is_the_lattice_mask():
    import torch

    from oakink2_tamf_amd.geometry import voxelize_lattice
    from oakink2_tamf_amd.meshdist import SDF_FIELDS, process_sdf

    v, f = mesh("twoparts")
    R = 24
    fields, info = process_sdf(v, f, 1.2, R, info=True)
    assert tuple(fields) == SDF_FIELDS
    ax = _ticks("twoparts", R)
    mask = voxelize_lattice(ax["verts_centred"], f, torch.from_numpy(ax["ticks"]).cuda()).reshape(-1).cpu().numpy()
    sdf = fields["sdf"]
    nz = sdf != 0
    assert np.array_equal((sdf > 0)[nz], mask[nz]) and info["n_inside"] == int(mask.sum())
    assert info["n_surface_points"] == int((mask & ~nz).sum())
    assert np.array_equal(np.abs(sdf), MR.mesh_distance(ax["verts_centred"], f, MR.lattice_points(ax["ticks"]))[0])
    assert np.array_equal(fields["point"], MR.lattice_points(ax["ticks"]) + ax["mesh_center"])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing():
    import torch
    from ctypes import c_void_p

    from oakink2_tamf_amd import meshdist as MD
    from oakink2_tamf_amd.hip_backend import _stream_ptr

    lib = MD._bind()
    ms = mesh_set(("twoparts",))
    dev = ms.device
    st = _stream_ptr(dev)
    ptr = lambda a: a.ctypes.data_as(c_void_p)  # noqa: E731
    msg = lambda: lib.tamf_meshdist_last_error().decode()  # noqa: E731
    ticks = torch.zeros((513, 3), dtype=torch.float64, device=dev)
    out = torch.full((64,), -7.0, dtype=torch.float64, device=dev)
    for R in (1, 513):
        assert lib.tamf_meshdist_lattice(ms._ws.data_ptr(), 1, 0, ticks.data_ptr(), R, 0, out.data_ptr(), st) == TAMF_ERR_INVALID
        assert f"R = {R}" in msg()
    assert lib.tamf_meshdist_lattice(ms._ws.data_ptr(), 1, 0, None, 4, 0, out.data_ptr(), st) == TAMF_ERR_INVALID and "null" in msg()
    assert lib.tamf_meshdist_lattice(ms._ws.data_ptr(), 1, 1, ticks.data_ptr(), 4, 0, out.data_ptr(), st) == TAMF_ERR_INVALID and "mesh = 1" in msg()
    assert lib.tamf_meshdist_lattice(ms._ws.data_ptr(), 1, 0, ticks.data_ptr(), 4, 2, out.data_ptr(), st) == TAMF_ERR_INVALID and "flags" in msg()

    pts = torch.zeros((10, 3), dtype=torch.float32, device=dev)
    face = torch.full((64,), -7, dtype=torch.int32, device=dev)
    ins = torch.full((64,), 9, dtype=torch.uint8, device=dev)
    jws = torch.zeros(64, dtype=torch.float64, device=dev)
    tr = np.ascontiguousarray(np.eye(3, 4).reshape(1, 12))

    def call(mid=0, off=0, ln=10, P=10, points=pts, dist=out, jbytes=512):
        a = [np.asarray([x], dtype=t) for x, t in ((mid, np.int32), (off, np.int64), (ln, np.int64))]
        return lib.tamf_meshdist_points(ms._ws.data_ptr(), 1, None if points is None else points.data_ptr(), P, 1, ptr(a[0]), ptr(tr), ptr(a[1]), ptr(a[2]),
                                        0, jws.data_ptr(), jbytes, None if dist is None else dist.data_ptr(), face.data_ptr(), ins.data_ptr(), st)

    assert call(mid=1) == TAMF_ERR_INVALID and "mesh_id[0] = 1" in msg()
    assert call(mid=-1) == TAMF_ERR_INVALID
    assert call(off=5, ln=6) == TAMF_ERR_INVALID and "leaves the 10 points" in msg()
    assert call(ln=-1) == TAMF_ERR_INVALID
    assert call(points=None) == TAMF_ERR_INVALID and "null" in msg()
    assert call(dist=None) == TAMF_ERR_INVALID and "null" in msg()
    assert call(jbytes=8) == TAMF_ERR_INVALID and "too small" in msg()
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (face == -7).all() and (ins == 9).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (out[:10] >= 0).all() and (out[10:] == -7.0).all()

    # a mesh with no valid face: the C entry points (an empty permutation slice) and the Python class
    v, f = C.flat_grid(2)
    f0 = np.ascontiguousarray(np.asarray([[0, 0, 1], [1, 2, 99]], dtype=np.int32))
    off1 = lambda n: np.asarray([0, n], dtype=np.int64)  # noqa: E731
    vo, fo, po = off1(len(v)), off1(2), off1(0)
    assert lib.tamf_meshdist_workspace(1, ptr(vo), ptr(fo), ptr(po)) == TAMF_ERR_INVALID and "no valid face" in msg()
    ws = torch.zeros(4096, dtype=torch.float64, device=dev)
    sc = np.ones((1, 3))
    perm = np.zeros(1, np.int32)
    assert lib.tamf_meshdist_prepare(ptr(v), ptr(f0), 1, ptr(vo), ptr(fo), ptr(perm), ptr(po), ptr(sc), ptr(sc), 512, ws.data_ptr(), 4096 * 8, st) == TAMF_ERR_INVALID
    po = off1(1)  # a face listed as valid that is not
    assert lib.tamf_meshdist_prepare(ptr(v), ptr(f0), 1, ptr(vo), ptr(fo), ptr(perm), ptr(po), ptr(sc), ptr(sc), 512, ws.data_ptr(), 4096 * 8, st) == TAMF_ERR_INVALID
    assert "listed as valid" in msg()
    torch.cuda.synchronize()
    assert (ws == 0).all()
    with pytest.raises(MD.MeshDistError, match="no valid face"):
        MD.MeshSet([(v, f0)])
