"""GPU: libtamf_eval.so - the lattice voxeliser and the batched counts against the brute-force tamf_mesh_contains and against what the
reference's own lines computed (tools/capture_siv_golden.py), exactly; clip_siv and the launcher against the per-frame loop of the
existing primitives; invariance of a job's count to the batch it is in; error paths; guard tails behind every output."""
import ctypes
import json
import os
import subprocess
import sys
from ctypes import c_void_p

import numpy as np
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
LATTICES = ["rotbox", "sphere", "torus", "twoparts", "aabox"]
CLIPS = ["two_objects", "skipped_object"]
INVALID = -1  # TAMF_ERR_INVALID
_cache = {}


def _lattice_fx(name):
    if ("fx", name) not in _cache:
        _cache[("fx", name)] = load_golden(f"siv_lattice_{name}.npz")
    return _cache[("fx", name)]


def _interior(name):
    """interior points of a fixture lattice from the captured reference mask (host only), + el_vol"""
    from oakink2_tamf_amd.metrics import siv

    if ("in", name) not in _cache:
        fx = _lattice_fx(name)
        R = int(fx["R"])
        ax = siv.lattice_axes(fx["verts"], 1.2, R)
        mask = np.unpackbits(fx["mask_packed"])[: R ** 3].astype(bool)
        pts = siv.lattice_points(ax["ticks"], ax["mesh_center"], np.nonzero(mask)[0])
        _cache[("in", name)] = siv.ObjectLattice(ax["mesh_center"], ax["extent"], ax["extent_expanded"], ax["tick_unit"], ax["ticks"], pts,
                                                 float(np.prod(ax["tick_unit"])), R, 1.2)
    return _cache[("in", name)]


def _transformed(tr12, p):
    """the query points of a job, float64, the order the kernel fixes"""
    M = np.asarray(tr12, np.float64).reshape(3, 4)
    return np.stack([((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + M[r, 3] for r in range(3)], axis=1)


def _composed_count(hand, faces, tr12, p):
    import torch

    from oakink2_tamf_amd import geometry

    if len(p) == 0:
        return 0
    return int(geometry.mesh_contains(np.asarray(hand, np.float32), faces, torch.from_numpy(_transformed(tr12, p)).cuda()).sum().item())


@pytest.mark.parametrize("R", [2, 37, 100])
@pytest.mark.parametrize("name", LATTICES)
def test_voxelize_equals_brute_force(name, R):
    import torch

    from oakink2_tamf_amd import geometry
    from oakink2_tamf_amd.metrics import siv

    fx = _lattice_fx(name)
    ax = siv.lattice_axes(fx["verts"], 1.2, R)
    got = geometry.voxelize_lattice(ax["verts_centred"], fx["faces"], torch.from_numpy(ax["ticks"]).cuda())
    x, y, z = np.meshgrid(ax["ticks"][:, 0], ax["ticks"][:, 1], ax["ticks"][:, 2], indexing="ij")
    q = np.vstack((x.flatten(), y.flatten(), z.flatten())).T
    want = geometry.mesh_contains(ax["verts_centred"], fx["faces"], torch.from_numpy(q).cuda())
    assert got.shape == (R, R, R) and got.dtype == torch.bool
    print(f"{name} R={R}: inside {int(want.sum())}")
    assert torch.equal(got.reshape(-1), want)


@pytest.mark.parametrize("name", LATTICES)
def test_voxelize_equals_the_reference_mask(name):
    """every fixture mesh at the R it was captured with (37, 48, 100), against the mask the reference's own lines produced"""
    import torch

    from oakink2_tamf_amd import geometry
    from oakink2_tamf_amd.metrics import siv

    fx = _lattice_fx(name)
    R = int(fx["R"])
    ax = siv.lattice_axes(fx["verts"], float(fx["bbox_expand_ratio"]), R)
    got = geometry.voxelize_lattice(ax["verts_centred"], fx["faces"], torch.from_numpy(ax["ticks"]).cuda())
    assert got.shape == (R, R, R)
    assert int(got.sum()) == int(fx["n_inside"])
    assert np.array_equal(np.packbits(got.reshape(-1).cpu().numpy()), fx["mask_packed"])
    lat = siv.object_lattice(fx["verts"], fx["faces"], resolution=R)
    assert np.array_equal(lat.points_in, _interior(name).points_in) and lat.el_vol == _interior(name).el_vol


@pytest.mark.parametrize("name", ["sphere", "aabox"])
def test_voxelize_large_r_and_odd_sizes(name):
    """R = 130 takes the 8-points-per-lane form (R > 128); 16 columns per work group do not divide 130^2"""
    import torch

    from oakink2_tamf_amd import geometry
    from oakink2_tamf_amd.metrics import siv

    fx = _lattice_fx(name)
    f = fx["faces"][:: 4 if name == "sphere" else 1]  # (an open surface is as good for equality; keeps the brute force short)
    ax = siv.lattice_axes(fx["verts"], 1.2, 130)
    got = geometry.voxelize_lattice(ax["verts_centred"], f, torch.from_numpy(ax["ticks"]).cuda())
    x, y, z = np.meshgrid(ax["ticks"][:, 0], ax["ticks"][:, 1], ax["ticks"][:, 2], indexing="ij")
    want = geometry.mesh_contains(ax["verts_centred"], f, torch.from_numpy(np.vstack((x.flatten(), y.flatten(), z.flatten())).T).cuda())
    assert torch.equal(got.reshape(-1), want) and int(want.sum()) > 0


def _clip(name):
    from oakink2_tamf_amd.metrics import siv

    fx = load_golden(f"siv_clip_{name}.npz")
    lattices = [_interior(str(o)) if has else None for o, has in zip(fx["obj_names"], fx["obj_has_lattice"])]
    jobs = siv.clip_jobs(int(fx["avai_len"]), [None if l is None else len(l.points_in) for l in lattices])
    return fx, lattices, jobs


@pytest.mark.parametrize("name", CLIPS)
def test_counts_equal_composition_and_reference(name):
    import torch

    from oakink2_tamf_amd import geometry

    fx, lattices, jobs = _clip(name)
    fr = fx["frames"]
    assert np.array_equal(jobs["frames"], fr)
    hands = np.stack([fx["hand_verts_gt"][fr], fx["hand_verts_refined"][fr]], axis=1).reshape(2 * len(fr), -1, 3)
    tr = fx["transf"][jobs["obj"], fr[jobs["frame_slot"]], :3, :].astype(np.float64)
    pts = np.concatenate([l.points_in for l in lattices if l is not None])
    got = geometry.mesh_contains_count(torch.from_numpy(hands).cuda(), fx["faces"], torch.from_numpy(pts).cuda(), jobs["pt_off"], jobs["pt_len"],
                                       jobs["mesh_id"], tr)
    assert got.dtype == torch.int64 and got.is_cuda
    got = got.cpu().numpy()
    want_ref = fx["counts"][jobs["frame_slot"], jobs["hand"], jobs["obj"]]
    comp = [_composed_count(hands[m], fx["faces"], t, pts[o: o + n]) for m, t, o, n in zip(jobs["mesh_id"], tr, jobs["pt_off"], jobs["pt_len"])]
    print(name, "counts", got.tolist())
    assert got.tolist() == comp
    assert np.array_equal(got, want_ref)


@pytest.mark.parametrize("name", CLIPS)
def test_clip_siv_equals_the_per_frame_loop_and_the_reference(name):
    import torch

    from oakink2_tamf_amd import geometry
    from oakink2_tamf_amd.metrics import siv

    fx, lattices, jobs = _clip(name)
    n = int(fx["avai_len"])
    g, r = siv.clip_siv(fx["hand_verts_gt"], fx["hand_verts_refined"], fx["faces"], fx["obj_traj"], lattices, n)
    loop = ([], [])
    for fr in range(0, n, 20):
        for h, hv in enumerate((fx["hand_verts_gt"], fx["hand_verts_refined"])):
            plist = [torch.from_numpy(_transformed(fx["transf"][k, fr, :3, :], l.points_in)).cuda() for k, l in enumerate(lattices) if l is not None]
            loop[h].append(geometry.solid_intersection_volume(hv[fr], fx["faces"], plist, [l.el_vol for l in lattices if l is not None]))
    assert [float(v) for v in g] == loop[0] and [float(v) for v in r] == loop[1]
    assert np.array_equal(np.asarray(g, np.float64), fx["gt_siv"]) and np.array_equal(np.asarray(r, np.float64), fx["refined_siv"])
    assert max(g) > 0.0


def _blobs(M, seed):
    from oracle.fixtures import icosphere

    v, f = icosphere(2)
    rng = np.random.default_rng(seed)
    out = [v * (1.0 + 0.15 * np.sin(3.0 * v[:, :1] + m)) * rng.uniform(0.02, 0.06, size=3) + rng.normal(scale=0.01, size=3) for m in range(M)]
    return np.asarray(out, np.float32), f.astype(np.int32)


@pytest.mark.parametrize("M", [1, 3, 64])
def test_job_invariance(M):
    """a job's count alone, inside 1 000 mixed jobs, and with the job order reversed: identical (and equal to the composition for a sample
    of jobs).  Covers empty slices, a mesh far from every point, and one slice above 2^20 points."""
    import torch

    from oakink2_tamf_amd import geometry

    rng = np.random.default_rng(100 + M)
    hands, faces = _blobs(M, M)
    if M > 1:
        hands[M - 1] += np.float32(50.0)  # none of the points is inside this one
    big = (1 << 20) + 777
    pts = np.concatenate([_interior("rotbox").points_in, _interior("twoparts").points_in, rng.normal(scale=0.03, size=(big, 3))])
    P = len(pts)
    J = 1000
    off = rng.integers(0, P - 6000, size=J)
    ln = rng.integers(1, 6000, size=J)
    ln[::17] = 0
    off[5], ln[5] = P - big, big  # the long slice: 2 049+ work groups of one job
    off[6], ln[6] = P, 0  # an empty slice at the very end
    mid = rng.integers(0, M, size=J).astype(np.int32)
    mid[7] = M - 1
    tr = np.zeros((J, 3, 4))
    for j in range(J):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        tr[j, :, :3], tr[j, :, 3] = q, rng.normal(scale=0.01, size=3)
    hv, pt = torch.from_numpy(hands).cuda(), torch.from_numpy(pts).cuda()
    full = geometry.mesh_contains_count(hv, faces, pt, off, ln, mid, tr).cpu().numpy()
    rev = geometry.mesh_contains_count(hv, faces, pt, off[::-1], ln[::-1], mid[::-1], tr[::-1]).cpu().numpy()
    assert np.array_equal(rev[::-1], full)
    assert (full[ln == 0] == 0).all() and (M == 1 or (full[mid == M - 1] == 0).all()) and full.max() > 0
    for j in (0, 1, 5, 6, 7, 17, 999):
        alone = geometry.mesh_contains_count(hv, faces, pt, off[j: j + 1], ln[j: j + 1], mid[j: j + 1], tr[j: j + 1]).cpu().numpy()
        assert alone[0] == full[j], j
        assert _composed_count(hands[mid[j]], faces, tr[j], pts[off[j]: off[j] + ln[j]]) == full[j], j
    print(f"M={M}: long slice count {full[5]}, total {int(full.sum())}")


# ---- the C interface directly: error paths and guard tails --------------------------------------------------------------------
def _eval():
    from oakink2_tamf_amd import geometry

    return geometry._bind_eval()


def test_error_paths_launch_nothing_and_guard_tails_hold():
    import torch

    from oakink2_tamf_amd.metrics import siv

    L = _eval()
    fx = _lattice_fx("rotbox")
    R = 37
    ax = siv.lattice_axes(fx["verts"], 1.2, R)
    v = torch.from_numpy(ax["verts_centred"]).cuda()
    f = torch.from_numpy(fx["faces"]).cuda()
    F = int(f.shape[0])
    tk = torch.from_numpy(ax["ticks"]).cuda()
    tri = ax["verts_centred"][fx["faces"]].reshape(-1, 3)
    scale = np.ascontiguousarray(511 / (tri.max(axis=0) - tri.min(axis=0)))
    transl = np.ascontiguousarray(0.5 - scale * tri.min(axis=0))
    ws = torch.empty(16 * F + 8, dtype=torch.float64, device="cuda")
    GUARD = 256
    out = torch.full((R ** 3 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    H = lambda a: a.ctypes.data_as(c_void_p)  # noqa: E731

    def vox(verts=P(v), faces=P(f), nf=F, ticks=P(tk), r=R, sc=H(scale), tl=H(transl), res=512, w=P(ws), o=P(out)):
        return L.tamf_voxelize_lattice(verts, faces, nf, ticks, r, sc, tl, res, w, o, c_void_p(0))

    for kw in (dict(r=1), dict(r=513), dict(nf=0), dict(verts=c_void_p(0)), dict(faces=c_void_p(0)), dict(ticks=c_void_p(0)), dict(sc=c_void_p(0)),
               dict(tl=c_void_p(0)), dict(w=c_void_p(0)), dict(o=c_void_p(0)), dict(res=1)):
        assert vox(**kw) == INVALID, kw
        assert L.tamf_eval_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())  # nothing was launched
    assert vox() == 0
    torch.cuda.synchronize()
    assert bool((out[R ** 3:] == 0xAB).all()) and int(out[: R ** 3].sum()) == int(fx["n_inside"])
    assert torch.isfinite(ws[: 16 * F]).all()

    hands, hf = _blobs(3, 9)
    hv, hfa = torch.from_numpy(hands).cuda(), torch.from_numpy(hf).cuda()
    pts = torch.from_numpy(_interior("rotbox").points_in).cuda()
    Pn, J, M, V, HF = int(pts.shape[0]), 4, 3, hands.shape[1], hf.shape[0]
    nbytes = L.tamf_mesh_contains_count_workspace(M, HF, J)
    assert nbytes == M * 64 + M * HF * 128 + J * 128
    assert L.tamf_mesh_contains_count_workspace(0, HF, J) == INVALID and L.tamf_mesh_contains_count_workspace(M, 0, J) == INVALID
    cws = torch.full((nbytes + GUARD,), 0xCD, dtype=torch.uint8, device="cuda")
    SENT = -0x0123456789ABCDEF
    cnt = torch.full((J + 8,), SENT, dtype=torch.int64, device="cuda")
    mid = np.array([0, 1, 2, 0], np.int32)
    off = np.array([0, 10, 0, Pn], np.int64)
    ln = np.array([Pn, 100, 0, 0], np.int64)
    tr = np.ascontiguousarray(np.tile(np.eye(3, 4).reshape(1, 12), (J, 1)))

    def count(verts=P(hv), m=M, faces=P(hfa), nf=HF, points=P(pts), pn=Pn, j=J, a_mid=mid, a_tr=H(tr), a_off=off, a_ln=ln, w=P(cws), wb=nbytes,
              o=P(cnt)):
        return L.tamf_mesh_contains_count(verts, m, V, faces, nf, points, pn, j, H(a_mid), a_tr, H(a_off), H(a_ln), 512, w, wb, o, c_void_p(0))

    bad_mid, neg_mid = mid.copy(), mid.copy()
    bad_mid[2], neg_mid[0] = M, -1
    past, past2, neg = ln.copy(), off.copy(), ln.copy()
    past[1], past2[3], neg[2] = Pn - 9, Pn + 1, -1
    for kw in (dict(a_mid=bad_mid), dict(a_mid=neg_mid), dict(a_ln=past), dict(a_off=past2), dict(a_ln=neg), dict(verts=c_void_p(0)),
               dict(faces=c_void_p(0)), dict(points=c_void_p(0)), dict(a_tr=c_void_p(0)), dict(w=c_void_p(0)), dict(o=c_void_p(0)),
               dict(wb=nbytes - 1), dict(m=0), dict(nf=0), dict(j=0)):
        assert count(**kw) == INVALID, kw
    torch.cuda.synchronize()
    assert bool((cnt == SENT).all()) and bool((cws == 0xCD).all())  # nothing was launched, nothing copied
    assert count() == 0
    torch.cuda.synchronize()
    assert bool((cnt[J:] == SENT).all()) and bool((cws[nbytes:] == 0xCD).all())
    got = cnt[:J].cpu().numpy()
    assert got[2] == 0 and got[3] == 0
    assert got[0] == _composed_count(hands[0], hf, tr[0], _interior("rotbox").points_in)
    assert got[1] == _composed_count(hands[1], hf, tr[1], _interior("rotbox").points_in[10:110])


# ---- launcher end to end ------------------------------------------------------------------------------------------------------
def test_launcher_end_to_end(tmp_path):
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fake_mano
    import test_score_cpu as S

    from oakink2_tamf_amd import geometry
    from oakink2_tamf_amd.launch import _score_common as C
    from oakink2_tamf_amd.launch import compute_score_siv as L
    from oakink2_tamf_amd.launch import formats
    from oakink2_tamf_amd.metrics import siv
    from oracle.fixtures import synthetic_object_mesh

    paths, _, tree = S._synthetic_tree(str(tmp_path))
    argv = ["--data.cache_dict_filepath", paths["cache"], "--data.obj_embedding_prefix", paths["emb"], "--data.obj_pointcloud_prefix", paths["pc"],
            "--debug.sample_refine_filepath", tree, "--mano.factory", "fake_mano:make", "--data.obj_model_loader",
            "oracle.fixtures:synthetic_object_mesh", "--out_json", str(tmp_path / "siv.json"), "--save_dir", str(tmp_path / "out")]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-m", "oakink2_tamf_amd.launch.compute_score_siv"] + argv, cwd=str(tmp_path), env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    printed = dict(l.split(" ", 1) for l in r.stdout.strip().splitlines() if " " in l)
    res = json.load(open(tmp_path / "siv.json"))
    # the same score by the per-frame loop over the existing primitives
    cfg = L.parse_args(argv)
    dev = torch.device("cuda:0")
    mano = fake_mano.make(None, dev)
    pairs = C.load_pairs(cfg, obj_model_loader=synthetic_object_mesh)
    items = [p[0] for p in pairs]
    _, gt_verts = C.ground_truth_mano(items, mano, dev, 64)
    lat = {}
    loop = ([], [])
    for (it, path), gv in zip(pairs, gt_verts):
        rv = np.asarray(formats.read_refine_sample(path)["verts"], np.float32)
        for k, o in enumerate(it["obj_list"]):
            if o not in lat:
                lat[o] = siv.object_lattice(it["obj_verts"][k], it["obj_faces"][k])
        faces = np.asarray(mano[2] if it["hand_side"] == "rh" else mano[3])
        tf = siv.tslrot6d_to_transf(np.asarray(it["obj_traj"])[:, : int(it["len"])])
        for fr in range(0, int(it["len"]), 20):
            for h, hv in enumerate((gv, rv)):
                plist = [torch.from_numpy(_transformed(tf[k, fr, :3, :], lat[o].points_in)).cuda() for k, o in enumerate(it["obj_list"])]
                loop[h].append(geometry.solid_intersection_volume(hv[fr], faces, plist, [lat[o].el_vol for o in it["obj_list"]]))
    assert res["n_frames"] == len(loop[0]) == int(printed["n_frames"]) and res["n_objects_skipped"] == 0 and res["n_clips"] == 3
    print("launcher", res["gt_siv"], res["refined_siv"])
    assert float(printed["gt_siv"]) == res["gt_siv"] == float(np.mean(loop[0]))
    assert float(printed["refined_siv"]) == res["refined_siv"] == float(np.mean(loop[1]))
    assert np.array_equal(np.load(tmp_path / "out" / "gt.npy"), np.asarray(loop[0])) and np.array_equal(np.load(tmp_path / "out" / "refined.npy"), np.asarray(loop[1]))
