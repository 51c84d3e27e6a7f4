"""GPU: the launchers with the winding-number sign, end to end on synthetic trees.  On closed meshes the flag changes no number, no
byte of an SDF file's `sdf` and no pixel; on a cube with a side removed the runs go through, report the sign, and what they call
inside is what tests/winding_restatement.py calls inside.  Without a flag the files are those of `--sign parity`."""
import json
import os
import pickle
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")) if p not in sys.path]

import winding_mesh_hook as H  # noqa: E402
import winding_restatement as WR  # noqa: E402

pytestmark = pytest.mark.gpu


def _decided(verts, faces, pts):
    """(inside by the longdouble restatement, mask of the points further than the gate from the threshold)"""
    _, wl, gate = WR.truth_and_gate(verts, faces, pts)
    with np.errstate(invalid="ignore"):
        return WR.inside(wl), np.abs(np.abs(wl) - 0.5) > gate


def test_process_object_sdf_sign_winding(tmp_path, capsys):
    from oakink2_tamf_amd import mesh_io
    from oakink2_tamf_amd.launch import process_object_sdf as P
    from oakink2_tamf_amd.meshdist import SDF_FIELDS
    from oakink2_tamf_amd.metrics import siv

    prefix = tmp_path / "meshes"
    os.makedirs(prefix)
    R = 24
    meshes = {}
    for name, is_open in (("closedcube", False), ("opencube", True)):
        mesh_io.write_ply(str(prefix / f"{name}.ply"), *H.turned_cube(open=is_open))
        meshes[name] = mesh_io.read_mesh(str(prefix / f"{name}.ply"))
    base = [str(prefix), "--resolution", str(R)]
    assert P.main(base + ["--out_dir", str(tmp_path / "default")]) == 0
    assert P.main(base + ["--out_dir", str(tmp_path / "parity"), "--sign", "parity", "--out_json", str(tmp_path / "parity.json")]) == 0
    capsys.readouterr()
    assert P.main(base + ["--out_dir", str(tmp_path / "winding"), "--sign", "winding", "--out_json", str(tmp_path / "winding.json")]) == 0
    io = capsys.readouterr()
    assert "sign winding" in io.out and "opencube: the mesh is not closed" in io.err and "the sign is the winding number's" in io.err
    assert "presumes a closed mesh" not in io.err and "closedcube: the mesh" not in io.err
    for name in meshes:  # without the flag: the files of --sign parity, byte for byte
        assert open(tmp_path / "default" / f"{name}.pkl", "rb").read() == open(tmp_path / "parity" / f"{name}.pkl", "rb").read()
    index = json.load(open(tmp_path / "winding.json"))
    assert index["sign"] == "winding" and [(o["obj_id"], o["sign"], o["closed"]) for o in index["objects"]] == [("closedcube", "winding", True), ("opencube", "winding", False)]
    assert json.load(open(tmp_path / "parity.json"))["sign"] == "parity"
    files = {}
    for kind in ("parity", "winding"):
        for name in meshes:
            d = pickle.load(open(tmp_path / kind / f"{name}.pkl", "rb"))
            assert tuple(d) == SDF_FIELDS and len(d) == 12 and d["sdf"].shape == (R ** 3,) and d["sdf"].dtype == np.float64
            files[kind, name] = d
    # the closed cube: the same sdf to the last bit, and every other field
    a, b = files["parity", "closedcube"], files["winding", "closedcube"]
    for k in SDF_FIELDS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert np.array_equal(a["sdf"].view(np.uint64), b["sdf"].view(np.uint64)) and (a["sdf"] > 0).any()
    # both cubes: sdf > 0 is the winding mask, which is the restatement's wherever that is decided - here everywhere
    for entry in index["objects"]:
        name = entry["obj_id"]
        v, f = meshes[name]
        ax = siv.lattice_axes(v, 1.2, R)
        want, decided = _decided(ax["verts_centred"], f, WR.lattice_points(ax["ticks"]))
        assert decided.all() and entry["n_surface_points"] == 0 and entry["n_inside"] == int(want.sum())
        got = files["winding", name]["sdf"] > 0
        assert np.array_equal(got, want), name
        assert np.array_equal(np.abs(files["winding", name]["sdf"]).view(np.uint64), np.abs(files["parity", name]["sdf"]).view(np.uint64))  # the distance is as before
    # the open cube: the lattice points the restatement puts inside ARE inside; ray parity loses the columns under the hole
    want, _ = _decided(siv.lattice_axes(meshes["opencube"][0], 1.2, R)["verts_centred"], meshes["opencube"][1],
                       WR.lattice_points(siv.lattice_axes(meshes["opencube"][0], 1.2, R)["ticks"]))
    par = files["parity", "opencube"]["sdf"] > 0
    assert want.sum() > 0 and (files["winding", "opencube"]["sdf"][want] > 0).all()
    print(f"open cube, {R}^3 lattice: winding inside {int(want.sum())}, ray parity inside {int(par.sum())}, of them in common {int((par & want).sum())}")
    # the SIV launcher's reader takes the file as it is
    lat = siv.load_sdf_pickle(str(tmp_path / "winding" / "opencube.pkl"))
    mem = siv.object_lattice(*meshes["opencube"], resolution=R, sign="winding")
    assert np.array_equal(lat.points_in, mem.points_in) and len(lat.points_in) == int(want.sum())
    ax = siv.lattice_axes(meshes["opencube"][0], 1.2, R)
    assert np.array_equal(mem.points_in, siv.lattice_points(ax["ticks"], ax["mesh_center"], np.flatnonzero(want)))  # the voxel set is the restatement's


def _pd_inputs(argv, loader):
    import torch

    import fake_mano
    from oakink2_tamf_amd.launch import _score_common as C
    from oakink2_tamf_amd.launch import compute_score_pd as L
    from oakink2_tamf_amd.launch import formats

    cfg = L.parse_args(argv)
    dev = torch.device("cuda:0")
    pairs = C.load_pairs(cfg, obj_model_loader=loader)
    items = [p[0] for p in pairs]
    _, gt_verts = C.ground_truth_mano(items, fake_mano.make(None, dev), dev, 64)
    return [(it, np.asarray(formats.read_refine_sample(path)["verts"], np.float32), gv) for (it, path), gv in zip(pairs, gt_verts)]


def test_compute_score_pd_sign_winding(tmp_path, capsys):
    import object_mesh_hook
    import test_score_cpu as S

    from oakink2_tamf_amd.launch import compute_score_pd as L
    from oakink2_tamf_amd.meshdist import MeshSet
    from oakink2_tamf_amd.metrics import pd as PD
    from oakink2_tamf_amd.metrics import siv
    from oakink2_tamf_amd.winding import WindingSet

    paths, _, tree = S._synthetic_tree(str(tmp_path))
    base = S._data_args(paths, tree) + ["--mano.factory", "fake_mano:make"]

    def run(tag, extra):
        capsys.readouterr()
        assert L.main(base + extra + ["--out_json", str(tmp_path / f"{tag}.json"), "--save_dir", str(tmp_path / tag)]) == 0
        printed = dict(l.split(" ", 1) for l in capsys.readouterr().out.strip().splitlines() if " " in l)
        return json.load(open(tmp_path / f"{tag}.json")), printed, np.load(tmp_path / tag / "gt.npy"), np.load(tmp_path / tag / "refined.npy")

    # closed objects: the same numbers to the last bit with and without the flag
    closed = ["--data.obj_model_loader", "object_mesh_hook:load_obj"]
    a, pa, ga, ra = run("plain", closed)
    b, pb, gb, rb = run("wind", closed + ["--sign", "winding"])
    assert a["sign"] == "parity" == pa["sign"] and b["sign"] == "winding" == pb["sign"]
    assert {k: v for k, v in a.items() if k != "sign"} == {k: v for k, v in b.items() if k != "sign"}
    assert np.array_equal(ga.view(np.uint64), gb.view(np.uint64)) and np.array_equal(ra.view(np.uint64), rb.view(np.uint64))
    # one object an open cube: the run goes through, reports the sign, and equals metrics/pd.py called directly
    opened = ["--data.obj_model_loader", "winding_mesh_hook:load_obj"]
    c, pc, gc, rc = run("open", opened + ["--sign", "winding"])
    assert c["sign"] == "winding" == pc["sign"] and c["n_objects_skipped"] == 0
    direct = ([], [])
    checked = n_inside = 0
    for it, rv, gv in _pd_inputs(base + opened, H.load_obj):
        meshes = [(it["obj_verts"][k], it["obj_faces"][k]) for k in range(len(it["obj_list"]))]
        ms, ws = MeshSet(meshes), WindingSet(meshes)
        ids = list(range(len(meshes)))
        depth, _ = PD.clip_pd(gv, rv, it["obj_traj"], ms, ids, int(it["len"]), sign="winding", winding_set=ws)
        direct[0].extend(depth[0].tolist())
        direct[1].extend(depth[1].tolist())
        # the jobs of clip_pd once more: `inside` is the restatement's on every vertex where that is decided
        n = int(it["len"])
        V = gv.shape[1]
        jobs = PD.clip_jobs(n, ids, V, PD.STRIDE)
        frames = jobs["frames"]
        hands = np.ascontiguousarray(np.stack([np.asarray(gv, np.float32)[:n][frames], rv[:n][frames]], axis=1).reshape(-1, 3))
        inv = PD.inverse_transf(siv.tslrot6d_to_transf(np.asarray(it["obj_traj"])[:, :n]))
        tr = inv[jobs["obj"], frames[jobs["frame_slot"]]].astype(np.float64)
        _, ins = ws.points(hands, jobs["mesh_id"], tr, jobs["pt_off"], jobs["pt_len"])
        ins = ins.cpu().numpy().reshape(len(jobs["mesh_id"]), V)
        for j in range(len(jobs["mesh_id"])):
            if it["obj_list"][int(jobs["obj"][j])] != H.OPEN_ID:
                continue
            q = WR.transform(hands[jobs["pt_off"][j]: jobs["pt_off"][j] + V], tr[j])
            want, decided = _decided(*meshes[int(jobs["mesh_id"][j])], q)
            assert np.array_equal(ins[j][decided], want[decided])
            checked += int(decided.sum())
            n_inside += int(want.sum())
    assert checked > 0
    assert np.array_equal(gc, np.asarray(direct[0])) and np.array_equal(rc, np.asarray(direct[1]))
    # the built-in mesh files with an open one: n_objects_open is still reported, it is a fact about the data
    ids = ["C10001", "O02@0007@00001", "S11005", "O02@0042@00003"]
    object_mesh_hook.write_prefix(str(tmp_path / "meshes"), ids, open_ids=("S11005",))
    d, pd_, _, _ = run("prefix", ["--data.obj_mesh_prefix", str(tmp_path / "meshes"), "--sign", "winding"])
    assert d["n_objects_open"] == 1 == int(pd_["n_objects_open"]) and d["objects_open"] == ["S11005"] and d["sign"] == "winding"
    print(f"pd --sign winding: {checked} vertices against the open cube checked, {n_inside} inside; refined_pd {c['refined_pd']!r} gt_pd {c['gt_pd']!r}")


def test_compute_score_siv_obj_sign_winding(tmp_path, capsys):
    import test_score_cpu as S

    from oakink2_tamf_amd.launch import compute_score_siv as L

    paths, _, tree = S._synthetic_tree(str(tmp_path))
    base = S._data_args(paths, tree) + ["--mano.factory", "fake_mano:make"]

    def run(tag, extra):
        capsys.readouterr()
        assert L.main(base + extra + ["--out_json", str(tmp_path / f"{tag}.json"), "--save_dir", str(tmp_path / tag)]) == 0
        printed = dict(l.split(" ", 1) for l in capsys.readouterr().out.strip().splitlines() if " " in l)
        return json.load(open(tmp_path / f"{tag}.json")), printed, np.load(tmp_path / tag / "gt.npy"), np.load(tmp_path / tag / "refined.npy")

    closed = ["--data.obj_model_loader", "object_mesh_hook:load_obj"]
    a, pa, ga, ra = run("plain", closed)
    b, pb, gb, rb = run("wind", closed + ["--data.obj_sign", "winding"])
    assert a["obj_sign"] == "parity" == pa["obj_sign"] and b["obj_sign"] == "winding" == pb["obj_sign"]
    assert {k: v for k, v in a.items() if k != "obj_sign"} == {k: v for k, v in b.items() if k != "obj_sign"}
    assert np.array_equal(ga.view(np.uint64), gb.view(np.uint64)) and np.array_equal(ra.view(np.uint64), rb.view(np.uint64))
    c, pc, gc, rc = run("open", ["--data.obj_model_loader", "winding_mesh_hook:load_obj", "--data.obj_sign", "winding"])
    assert c["obj_sign"] == "winding" == pc["obj_sign"] and c["n_objects_skipped"] == 0 and c["n_frames"] == a["n_frames"]
    assert np.isfinite(gc).all() and np.isfinite(rc).all()
    print("siv --data.obj_sign winding:", a["gt_siv"], b["gt_siv"], c["gt_siv"])
    # (that the open cube's voxel set is the restatement's: test_process_object_sdf_sign_winding, through siv.object_lattice)


def test_render_penetration_sign_winding(tmp_path, monkeypatch):
    import test_render_launch_gpu as RL

    from oakink2_tamf_amd.launch import render_samples as RS

    monkeypatch.setattr(RL, "OBJ_SHIFT", ((0.09, 0.0, 0.0), (0.30, 0.0, 0.0)))  # the first object of every clip INTO the hand (test_pd_launch_gpu)
    paths, cache, tree = RL._tree(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    data = ["--data.cache_dict_filepath", paths["cache"], "--data.obj_embedding_prefix", paths["emb"], "--data.obj_pointcloud_prefix", paths["pc"],
            "--debug.sample_refine_filepath", tree, "--render.width", "64", "--render.height", "64", "--data.obj_model_loader",
            "oracle.fixtures:synthetic_object_mesh", "--with_gt", "--mano.factory", "fake_mano:make", "--render.every", "6", "--render.penetration_map"]
    assert RS.main(data + ["--out_dir", str(tmp_path / "parity"), "--out_json", str(tmp_path / "parity.json")]) == 0
    assert RS.main(data + ["--render.penetration_sign", "winding", "--out_dir", str(tmp_path / "winding"), "--out_json", str(tmp_path / "winding.json")]) == 0
    par, win = json.load(open(tmp_path / "parity.json")), json.load(open(tmp_path / "winding.json"))
    assert par["penetration"] == {"far_mm": 10.0} and win["penetration"] == {"far_mm": 10.0, "sign": "winding"}
    n = 0
    for cp, cw in zip(par["clips"], win["clips"]):
        assert cp["frames"] == cw["frames"]
        names = sorted(f for f in os.listdir(cp["dir"]) if f.endswith(".png"))
        assert names == sorted(f for f in os.listdir(cw["dir"]) if f.endswith(".png")) and names
        for name in names:  # closed meshes: the same pictures, byte for byte
            assert open(os.path.join(cp["dir"], name), "rb").read() == open(os.path.join(cw["dir"], name), "rb").read(), (cp["dir"], name)
            n += 1
    assert n > 0
