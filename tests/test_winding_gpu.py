"""libtamf_winding.so and oakink2_tamf_amd/winding.py on the GPU against tests/winding_restatement.py (include/tamf_winding.h in numpy).
atan2 is the one operation the header does not define bit for bit, so w is compared with a gate: for a case with F valid faces,
max(4 e_ref, F 2^-53), e_ref the largest difference between the float64 and the longdouble restatement over the case's points (the
longdouble run is the truth).  Everything the header does define is compared in bits: the two routes of the points call, a job alone
and in a batch, the lattice form and the points form, the same call twice."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")) if p not in sys.path]

import meshdist_cases as C  # noqa: E402
import winding_restatement as WR  # noqa: E402

pytestmark = pytest.mark.gpu

TAMF_ERR_INVALID = -1


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name in C.FIXTURES:
        return C.fixture_mesh(name)
    if name.startswith("bumpy"):
        return C.bumpy_grid(int(name[5:]))
    if name.startswith("flat"):
        return C.flat_grid(int(name[4:]))
    if name == "broken":
        v, f, _ = C.with_invalid_faces(*C.fixture_mesh("twoparts"))
        return v, f
    if name == "uvsphere":
        return WR.uv_sphere(16, 32, 0.05)
    raise KeyError(name)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def pose(seed):
    return C.IDENTITY if seed is None else C.rigid(seed)


@functools.lru_cache(maxsize=None)
def points(name, n, seed):
    return C.points_around(mesh(name)[0], n, seed)


@functools.lru_cache(maxsize=None)
def reference(name, n, seed, pose_seed):
    """(truth w in longdouble, gate) by the restatement at the header's query points, computed once and shared (do not modify)"""
    v, f = mesh(name)
    q = WR.transform(points(name, n, seed), pose(pose_seed))
    _, wl, gate = WR.truth_and_gate(v, f, q)
    return wl, gate


@functools.lru_cache(maxsize=None)
def winding_set(names):
    from oakink2_tamf_amd.winding import WindingSet

    return WindingSet([mesh(n) for n in names])


def run_jobs(names, jobs, route=None, inside=True):
    """jobs: [(mesh name, n, seed, pose seed)] -> per job (w, inside) as numpy, one call"""
    pts = [points(j[0], j[1], j[2]) if j[1] else np.zeros((0, 3), np.float32) for j in jobs]
    ln = np.asarray([len(p) for p in pts], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)
    ws = winding_set(tuple(names))
    w, i = ws.points(np.concatenate(pts), [names.index(j[0]) for j in jobs], np.stack([pose(j[3]) for j in jobs]), off, ln, inside=inside, route=route)
    w = w.cpu().numpy()
    i = i.cpu().numpy() if inside else None
    o = np.concatenate([[0], np.cumsum(ln)])
    return [(w[o[k]:o[k + 1]], None if i is None else i[o[k]:o[k + 1]]) for k in range(len(jobs))]


def check_against_truth(tag, w, ins, wl, gate):
    """w within the gate of the truth; inside equal to the truth's wherever the truth is further than the gate from the threshold,
    which on these inputs is everywhere"""
    err = float(np.abs(w.astype(np.longdouble) - wl).max()) if w.size else 0.0
    margin = float(np.abs(np.abs(wl) - 0.5).min()) if w.size else 1.0
    print(f"{tag}: largest device error {err:.3e}, gate {gate:.3e}, smallest | |w| - 0.5 | {margin:.3e}")
    assert margin > gate, (tag, margin, gate)
    assert err <= gate, (tag, err, gate)
    if ins is not None:
        assert np.array_equal(ins, WR.inside(wl)), tag


# face counts 1, 63, chunk - 1, chunk, chunk + 1, 2 chunks + 1, 5 chunks (closed), one with invalid faces interleaved;
# point counts 1, 255, 256, 257, 1000; poses
FACE_CASES = [("flat1", 257, 21, None), ("bumpy63", 1, 22, 1), ("bumpy1023", 255, 23, None), ("bumpy1024", 256, 24, 2), ("bumpy1025", 1000, 25, 3),
              ("bumpy2049", 257, 26, None), ("sphere", 1000, 27, 4), ("broken", 256, 28, 5)]


@pytest.mark.parametrize("job", FACE_CASES, ids=[j[0] for j in FACE_CASES])
def test_face_and_point_counts(job):
    v, f = mesh(job[0])
    assert WR.n_valid(v, f) == {"flat1": 1, "bumpy63": 63, "bumpy1023": 1023, "bumpy1024": 1024, "bumpy1025": 1025, "bumpy2049": 2049, "sphere": 5120,
                                "broken": 332}[job[0]]
    wl, gate = reference(*job)
    w, ins = run_jobs([job[0]], [job])[0]
    check_against_truth(job[0], w, ins, wl, gate)
    for route in ("loop", "spread"):  # the same tree, the same bits
        w2, ins2 = run_jobs([job[0]], [job], route=route)[0]
        assert np.array_equal(bits(w2), bits(w)) and np.array_equal(ins2, ins), (job, route)


def _ticks(name, R):
    """(R, 3) float64 ticks over the mesh's box grown by 1.2, rounded to float32 values (the points form takes float32)"""
    v = mesh(name)[0]
    lo, hi = v.min(0), v.max(0)
    c, h = (lo + hi) / 2, (hi - lo) / 2 * 1.2 + 0.01
    return np.linspace(c - h, c + h, R).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def lattice_reference(name, R):
    v, f = mesh(name)
    tk = WR.sphere_lattice(0.05, R, 1.2) if name == "uvsphere" else _ticks(name, R)
    pts = WR.lattice_points(tk)
    _, wl, gate = WR.truth_and_gate(v, f, pts)
    return tk, pts, wl, gate


@pytest.mark.parametrize("name,R", [("bumpy1025", 2), ("bumpy2049", 5), ("uvsphere", 24)])
def test_lattice_matches_restatement_and_points_form(name, R):
    tk, pts, wl, gate = lattice_reference(name, R)
    ws = winding_set((name,))
    w, ins = ws.lattice(0, tk)
    assert w.shape == (R, R, R) and ins.shape == (R, R, R)
    w, ins = w.cpu().numpy().reshape(-1), ins.cpu().numpy().reshape(-1)
    check_against_truth(f"lattice {name} R={R}", w, ins, wl, gate)
    for route in ("loop", "spread"):
        wp, ip = ws.points(pts.astype(np.float32), [0], route=route)
        assert np.array_equal(bits(wp.cpu().numpy()), bits(w)) and np.array_equal(ip.cpu().numpy(), ins), route
    w_only, none = ws.lattice(0, tk, inside=False)
    assert none is None and np.array_equal(bits(w_only.cpu().numpy().reshape(-1)), bits(w))


# ---- determinism and batch independence -----------------------------------------------------------------------------------------------
BATCH_NAMES = ["bumpy2049", "sphere", "bumpy63"]
BATCH = [("sphere", 257, 31, 6), ("bumpy63", 1000, 32, None), ("bumpy2049", 0, 33, 7), ("bumpy2049", 255, 34, 8), ("sphere", 1, 35, None),
         ("bumpy63", 256, 36, 9), ("bumpy2049", 257, 26, None), ("sphere", 64, 37, 10), ("bumpy63", 7, 38, 11), ("bumpy2049", 300, 39, 12)]


def test_same_bits_twice_alone_in_a_batch_and_on_either_route():
    ref = run_jobs(BATCH_NAMES, BATCH, route="loop")
    assert ref[2][0].size == 0 and ref[2][1].size == 0
    for route in (None, "loop", "spread"):
        got = run_jobs(BATCH_NAMES, BATCH, route=route)
        for k, (a, b) in enumerate(zip(got, ref)):
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]), (route, k)
    for k in (0, 3, 6, 9):  # a job by itself, on a set of its own, against the same job among the nine others
        for route in ("loop", "spread"):
            alone = run_jobs([BATCH[k][0]], [BATCH[k]], route=route)[0]
            assert np.array_equal(bits(alone[0]), bits(ref[k][0])) and np.array_equal(alone[1], ref[k][1]), (k, route)
    wl, gate = reference(*BATCH[6])  # (shared with test_face_and_point_counts)
    check_against_truth("batched bumpy2049", ref[6][0], ref[6][1], wl, gate)


def test_transformed_job_equals_identity_job_on_transformed_points():
    """a transform whose arithmetic is exact in float32 and float64 alike: permutation with signs, scale 2, dyadic translation"""
    name = "bumpy1025"
    p = (np.round(points(name, 300, 41) * 64) / 64).astype(np.float32)
    t = np.asarray([[0.0, -2.0, 0.0, 0.25], [0.0, 0.0, 2.0, -0.5], [2.0, 0.0, 0.0, 0.125]])
    q = WR.transform(p, t)
    q32 = q.astype(np.float32)
    assert np.array_equal(q32.astype(np.float64), q)
    ws = winding_set((name,))
    for route in ("loop", "spread"):
        a, ia = ws.points(p, [0], t.reshape(1, 12), route=route)
        b, ib = ws.points(q32, [0], route=route)
        assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())) and np.array_equal(ia.cpu().numpy(), ib.cpu().numpy())


# ---- edge inputs --------------------------------------------------------------------------------------------------------------------
def test_surface_points_nan_points_and_nan_transforms():
    name = "flat63"
    v, f = mesh(name)
    on, kind = C.on_surface_points(v, f)
    ws = winding_set((name,))
    for route in ("loop", "spread"):
        w, _ = ws.points(on, [0], route=route)
        w = w.cpu().numpy()
        assert np.isfinite(w).all() and (np.abs(w) <= 0.5 * len(f)).all()
    sph = winding_set(("sphere",))
    w, _ = sph.points(mesh("sphere")[0].astype(np.float32), [0])  # (the rounded vertices: on or next to the surface)
    assert np.isfinite(w.cpu().numpy()).all()
    p = points("sphere", 257, 43).copy()
    p[[0, 100, 256], [0, 1, 2]] = np.nan
    for route in ("loop", "spread"):
        w, ins = sph.points(p, [0], route=route)
        w, ins = w.cpu().numpy(), ins.cpu().numpy()
        bad = np.zeros(257, bool)
        bad[[0, 100, 256]] = True
        assert np.isnan(w[bad]).all() and not ins[bad].any() and np.isfinite(w[~bad]).all()
        t = np.stack([C.IDENTITY, C.IDENTITY]).reshape(2, 12).copy()
        t[1, 5] = np.nan
        w, ins = sph.points(points("sphere", 257, 43), [0, 0], t, route=route)
        w, ins = w.cpu().numpy(), ins.cpu().numpy()
        assert np.isfinite(w[:257]).all() and np.isnan(w[257:]).all() and not ins[257:].any()


def test_outputs_land_in_their_slices_only():
    import torch
    from ctypes import c_void_p

    from oakink2_tamf_amd import winding as W
    from oakink2_tamf_amd.hip_backend import _stream_ptr

    lib = W._bind()
    ws = winding_set(("bumpy2049",))
    dev = ws.device
    st = _stream_ptr(dev)
    ptr = lambda a: a.ctypes.data_as(c_void_p)  # noqa: E731
    p = torch.from_numpy(points("bumpy2049", 300, 39)).to(dev)
    mid = np.zeros(2, np.int32)
    tr = np.ascontiguousarray(np.tile(np.eye(3, 4).reshape(1, 12), (2, 1)))
    off, ln = np.asarray([0, 43], np.int64), np.asarray([43, 257], np.int64)
    ref = run_jobs(["bumpy2049"], [("bumpy2049", 300, 39, None)], route="loop")[0]
    for flags in (1, 2):
        wbuf = torch.full((300 + 64,), -7.0, dtype=torch.float64, device=dev)
        ibuf = torch.full((300 + 64,), 9, dtype=torch.uint8, device=dev)
        jbytes = lib.tamf_winding_points_workspace(2, 1, ptr(mid), ptr(ln), ptr(ws.valid_off), flags)
        assert jbytes >= 2 * 144
        jws = torch.full((jbytes // 8 + 2 + 8,), -3.0, dtype=torch.float64, device=dev)
        rc = lib.tamf_winding_points(ws._ws.data_ptr(), 1, p.data_ptr(), 300, 2, ptr(mid), ptr(tr), ptr(off), ptr(ln), ptr(ws.valid_off), flags,
                                     jws.data_ptr(), jbytes, wbuf[32:].data_ptr(), ibuf[32:].data_ptr(), st)
        assert rc == 0, lib.tamf_winding_last_error()
        torch.cuda.synchronize()
        assert (wbuf[:32] == -7.0).all() and (wbuf[332:] == -7.0).all() and (ibuf[:32] == 9).all() and (ibuf[332:] == 9).all()
        assert (jws[jbytes // 8:] == -3.0).all()
        assert np.array_equal(bits(wbuf[32:332].cpu().numpy()), bits(ref[0])) and np.array_equal(ibuf[32:332].cpu().numpy().astype(bool), ref[1])
    # the lattice: R^3 outputs and not one more
    tk = torch.from_numpy(_ticks("bumpy2049", 5)).to(dev)
    wbuf = torch.full((125 + 64,), -7.0, dtype=torch.float64, device=dev)
    ibuf = torch.full((125 + 64,), 9, dtype=torch.uint8, device=dev)
    assert lib.tamf_winding_lattice(ws._ws.data_ptr(), 1, 0, tk.data_ptr(), 5, wbuf[32:].data_ptr(), ibuf[32:].data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert (wbuf[:32] == -7.0).all() and (wbuf[157:] == -7.0).all() and (ibuf[:32] == 9).all() and (ibuf[157:] == 9).all()
    assert (wbuf[32:157] != -7.0).all() and (ibuf[32:157] <= 1).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing():
    import torch
    from ctypes import c_void_p

    from oakink2_tamf_amd import winding as W
    from oakink2_tamf_amd.hip_backend import _stream_ptr

    lib = W._bind()
    ws = winding_set(("twoparts",))
    dev = ws.device
    st = _stream_ptr(dev)
    ptr = lambda a: a.ctypes.data_as(c_void_p)  # noqa: E731
    msg = lambda: lib.tamf_winding_last_error().decode()  # noqa: E731
    ticks = torch.zeros((513, 3), dtype=torch.float64, device=dev)
    out = torch.full((64,), -7.0, dtype=torch.float64, device=dev)
    ins = torch.full((64,), 9, dtype=torch.uint8, device=dev)
    for R in (1, 513):
        assert lib.tamf_winding_lattice(ws._ws.data_ptr(), 1, 0, ticks.data_ptr(), R, out.data_ptr(), ins.data_ptr(), st) == TAMF_ERR_INVALID
        assert f"R = {R}" in msg()
    assert lib.tamf_winding_lattice(ws._ws.data_ptr(), 1, 0, None, 4, out.data_ptr(), ins.data_ptr(), st) == TAMF_ERR_INVALID and "null" in msg()
    assert lib.tamf_winding_lattice(ws._ws.data_ptr(), 1, 1, ticks.data_ptr(), 4, out.data_ptr(), ins.data_ptr(), st) == TAMF_ERR_INVALID and "mesh = 1" in msg()
    assert lib.tamf_winding_lattice(ws._ws.data_ptr(), 1, 0, ticks.data_ptr(), 4, None, ins.data_ptr(), st) == TAMF_ERR_INVALID and "null" in msg()

    pts = torch.zeros((10, 3), dtype=torch.float32, device=dev)
    jws = torch.zeros(64, dtype=torch.float64, device=dev)
    tr = np.ascontiguousarray(np.eye(3, 4).reshape(1, 12))

    def call(mid=0, off=0, ln=10, P=10, points=pts, w=out, jbytes=512, flags=0, jshift=0, voff=ws.valid_off):
        a = [np.asarray([x], dtype=t) for x, t in ((mid, np.int32), (off, np.int64), (ln, np.int64))]
        return lib.tamf_winding_points(ws._ws.data_ptr(), 1, None if points is None else points.data_ptr(), P, 1, ptr(a[0]), ptr(tr), ptr(a[1]), ptr(a[2]),
                                       None if voff is None else ptr(voff), flags, jws.data_ptr() + jshift, jbytes, None if w is None else w.data_ptr(),
                                       ins.data_ptr(), st)

    assert call(mid=1) == TAMF_ERR_INVALID and "mesh_id[0] = 1" in msg()
    assert call(mid=-1) == TAMF_ERR_INVALID
    assert call(off=5, ln=6) == TAMF_ERR_INVALID and "leaves the 10 points" in msg()
    assert call(ln=-1) == TAMF_ERR_INVALID
    assert call(points=None) == TAMF_ERR_INVALID and "null" in msg()
    assert call(w=None) == TAMF_ERR_INVALID and "null" in msg()
    assert call(voff=None) == TAMF_ERR_INVALID and "null" in msg()
    assert call(jbytes=8) == TAMF_ERR_INVALID and "too small" in msg()
    assert call(jshift=8) == TAMF_ERR_INVALID and "16-byte aligned" in msg()
    assert call(flags=3) == TAMF_ERR_INVALID and "both routes" in msg()
    assert call(flags=4) == TAMF_ERR_INVALID and "unknown flags" in msg()
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (ins == 9).all() and (jws == 0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (out[:10] != -7.0).all() and (out[10:] == -7.0).all() and (ins[:10] <= 1).all() and (ins[10:] == 9).all()

    # prepare: a misaligned or small workspace, a list that is not ascending, a face listed as valid that is not; no valid face
    v, f = mesh("twoparts")
    f = np.ascontiguousarray(f)
    off1 = lambda n: np.asarray([0, n], dtype=np.int64)  # noqa: E731
    vo, fo = off1(len(v)), off1(len(f))
    wsb = torch.zeros(8192, dtype=torch.float64, device=dev)
    good = np.arange(len(f), dtype=np.int32)
    prep = lambda valid, shift=0, nbytes=8192 * 8 - 16: lib.tamf_winding_prepare(ptr(v), ptr(f), 1, ptr(vo), ptr(fo), ptr(valid), ptr(off1(len(valid))),  # noqa: E731
                                                                                 wsb.data_ptr() + shift, nbytes, st)
    assert prep(good, shift=8) == TAMF_ERR_INVALID and "16-byte aligned" in msg()
    assert prep(good, nbytes=64) == TAMF_ERR_INVALID and "too small" in msg()
    assert prep(good[::-1].copy()) == TAMF_ERR_INVALID and "not strictly ascending" in msg()
    assert prep(np.asarray([0, 1, len(f)], np.int32)) == TAMF_ERR_INVALID and "outside [0," in msg()
    f_bad = f.copy()
    f_bad[1, 2] = f_bad[1, 1]
    assert lib.tamf_winding_prepare(ptr(v), ptr(f_bad), 1, ptr(vo), ptr(fo), ptr(good), ptr(fo), wsb.data_ptr(), 8192 * 8, st) == TAMF_ERR_INVALID
    assert "listed as valid" in msg()
    assert lib.tamf_winding_workspace(1, ptr(vo), ptr(fo), ptr(off1(0))) == TAMF_ERR_INVALID and "no valid face" in msg()
    torch.cuda.synchronize()
    assert (wsb == 0).all()
    assert prep(good) == 0

    # from Python
    with pytest.raises(ValueError, match="float32"):
        ws.points(np.zeros((4, 3), np.float64), [0])
    with pytest.raises(W.WindingError, match="mesh_id"):
        ws.points(np.zeros((4, 3), np.float32), [1])
    with pytest.raises(W.WindingError, match="leaves the 4 points"):
        ws.points(np.zeros((4, 3), np.float32), [0], pt_off=[2], pt_len=[3])
    with pytest.raises(W.WindingError, match="R = 1"):
        ws.lattice(0, np.zeros((1, 3)))
    with pytest.raises(ValueError, match="route"):
        ws.points(np.zeros((4, 3), np.float32), [0], route="fast")
    with pytest.raises(W.WindingError, match="no valid face"):
        W.WindingSet([(v, np.asarray([[0, 0, 1], [1, 2, 9999]], np.int32))])


# ---- against the old sign ---------------------------------------------------------------------------------------------------------------
def test_closed_mesh_turned_out_of_the_axes_agrees_with_ray_parity():
    import torch

    from oakink2_tamf_amd.geometry import voxelize_lattice
    from oakink2_tamf_amd.winding import lattice_winding

    v, f = mesh("rotbox")
    tk = torch.from_numpy(_ticks("rotbox", 24)).cuda()
    _, ins = lattice_winding(v, f, tk)
    old = voxelize_lattice(v, f, tk)
    assert ins.shape == old.shape == (24, 24, 24) and 0 < int(old.sum()) < 24 ** 3
    assert torch.equal(ins, old.bool())


def test_uv_sphere_with_poles_on_z_winding_is_right_where_ray_parity_is_not():
    import torch

    from oakink2_tamf_amd.geometry import voxelize_lattice

    v, f = mesh("uvsphere")
    tk, pts, wl, gate = lattice_reference("uvsphere", 24)
    r = np.linalg.norm(pts, axis=1)
    r_in = WR.inscribed_radius(v, f)
    band = (r >= r_in) & (r <= 0.05)
    assert band.mean() <= 0.03
    want = r < r_in
    _, ins = winding_set(("uvsphere",)).lattice(0, tk)
    ins = ins.cpu().numpy().reshape(-1)
    assert np.array_equal(ins[~band], want[~band])
    old = voxelize_lattice(v, f, torch.from_numpy(tk).cuda()).cpu().numpy().reshape(-1).astype(bool)
    print(f"uv sphere, poles on z, 24^3 lattice: ray parity wrong on {int((old != want)[~band].sum())} of {int((~band).sum())} points outside the band, "
          f"winding on {int((ins != want)[~band].sum())}")
