"""GPU: the launchers around the point-to-mesh distance end to end on synthetic trees - compute_score_pd against metrics/pd.py called
directly (a loader hook, a mesh prefix with an open mesh, an object without a usable mesh), process_object_sdf's pickles through
compute_score_siv's reader against the in-memory lattice (the same SIV to the last bit), and render_samples' penetration map against
the restated depths, with the frames of a run without the flag byte for byte what the existing API renders."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")) if p not in sys.path]

import meshdist_restatement as MR  # noqa: E402

pytestmark = pytest.mark.gpu


def _direct_pd(argv, loader, stride=20):
    """the score by metrics/pd.py called directly on the launcher's inputs -> (gt, refined, gt_pen, refined_pen, skipped ids)"""
    import torch

    import fake_mano
    from oakink2_tamf_amd.launch import _score_common as C
    from oakink2_tamf_amd.launch import compute_score_pd as L
    from oakink2_tamf_amd.launch import formats
    from oakink2_tamf_amd.meshdist import MeshDistError, MeshSet
    from oakink2_tamf_amd.metrics import pd as PD

    cfg = L.parse_args(argv)
    dev = torch.device("cuda:0")
    pairs = C.load_pairs(cfg, obj_model_loader=loader)
    items = [p[0] for p in pairs]
    _, gt_verts = C.ground_truth_mano(items, fake_mano.make(None, dev), dev, 64)
    out = ([], [], [], [])
    skipped = []
    for (it, path), gv in zip(pairs, gt_verts):
        rv = np.asarray(formats.read_refine_sample(path)["verts"], np.float32)
        meshes, ids = [], []
        for k, o in enumerate(it["obj_list"]):
            try:
                MeshSet([(it["obj_verts"][k], it["obj_faces"][k])], upload=False)
                ids.append(len(meshes))
                meshes.append((it["obj_verts"][k], it["obj_faces"][k]))
            except MeshDistError:
                ids.append(None)
                if o not in skipped:
                    skipped.append(o)
        depth, pen = PD.clip_pd(gv, rv, it["obj_traj"], MeshSet(meshes) if meshes else None, ids, int(it["len"]), stride=stride)  # a set per clip
        for k, a in enumerate((depth[0], depth[1], pen[0], pen[1])):
            out[k].extend(a.tolist())
    return out + (skipped,)


def _check(res, printed, direct, save_dir):
    from oakink2_tamf_amd.metrics import pd as PD

    g, r, gp, rp, skipped = direct
    want = PD.summary(g, r, gp, rp)
    assert res["n_frames"] == len(g) == int(printed["n_frames"]) and res["objects_skipped"] == skipped and int(printed["n_objects_skipped"]) == len(skipped)
    for key, val in want.items():
        assert res[key] == val == float(printed[key]), key
    assert np.array_equal(np.load(os.path.join(save_dir, "gt.npy")), np.asarray(g)) and np.array_equal(np.load(os.path.join(save_dir, "refined.npy")), np.asarray(r))


def test_pd_launcher_end_to_end(tmp_path, capsys):
    import object_mesh_hook
    import pd_mesh_hook
    import test_score_cpu as S

    from oakink2_tamf_amd.launch import compute_score_pd as L

    paths, _, tree = S._synthetic_tree(str(tmp_path))
    base = S._data_args(paths, tree) + ["--mano.factory", "fake_mano:make"]
    # 1: a loader hook, as a process of its own
    argv = base + ["--data.obj_model_loader", "object_mesh_hook:load_obj", "--out_json", str(tmp_path / "pd.json"), "--save_dir", str(tmp_path / "out")]
    r = S._launch("compute_score_pd", argv, str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    printed = dict(l.split(" ", 1) for l in r.stdout.strip().splitlines() if " " in l)
    res = json.load(open(tmp_path / "pd.json"))
    assert res["n_clips"] == 3 and res["n_objects"] == 4 and res["n_objects_skipped"] == 0 and res["stride"] == 20 and "n_objects_open" not in res
    assert res["n_frames"] == 8 + 1 + 5  # lens 160, 16, 97
    direct = _direct_pd(argv, object_mesh_hook.load_obj)
    _check(res, printed, direct, str(tmp_path / "out"))
    print("pd launcher", {k: res[k] for k in ("gt_pd", "refined_pd", "gt_pd_max", "refined_pd_max", "gt_pen_frame_ratio", "refined_pen_frame_ratio")})
    # 2: an object whose mesh has no valid face is left out and counted; another stride (in this process)
    capsys.readouterr()
    argv = base + ["--data.obj_model_loader", "pd_mesh_hook:load_obj", "--stride", "7", "--out_json", str(tmp_path / "pd2.json"), "--save_dir", str(tmp_path / "out2")]
    assert L.main(argv) == 0
    printed = dict(l.split(" ", 1) for l in capsys.readouterr().out.strip().splitlines() if " " in l)
    res = json.load(open(tmp_path / "pd2.json"))
    assert res["objects_skipped"] == [pd_mesh_hook.NO_MESH] and res["n_objects_skipped"] == 1 and res["stride"] == 7 and res["n_frames"] == 23 + 3 + 14
    _check(res, printed, _direct_pd(argv, pd_mesh_hook.load_obj, stride=7), str(tmp_path / "out2"))
    # 3: the built-in mesh files, one of them open: the same figures as the hook on the closed ones, and the open one is named
    ids = ["C10001", "O02@0007@00001", "S11005", "O02@0042@00003"]
    object_mesh_hook.write_prefix(str(tmp_path / "meshes"), ids, open_ids=("S11005",))
    argv = base + ["--data.obj_mesh_prefix", str(tmp_path / "meshes"), "--out_json", str(tmp_path / "pd3.json"), "--save_dir", str(tmp_path / "out3")]
    assert L.main(argv) == 0
    printed = dict(l.split(" ", 1) for l in capsys.readouterr().out.strip().splitlines() if " " in l)
    res3 = json.load(open(tmp_path / "pd3.json"))
    assert res3["n_objects_open"] == 1 == int(printed["n_objects_open"]) and res3["objects_open"] == ["S11005"] and res3["n_objects_skipped"] == 0
    from oakink2_tamf_amd import mesh_io

    _check(res3, printed, _direct_pd(argv, mesh_io.directory_loader(str(tmp_path / "meshes"))), str(tmp_path / "out3"))


def test_sdf_pickles_give_the_same_siv_as_the_in_memory_lattice(tmp_path, capsys):
    from conftest import load_golden
    from oakink2_tamf_amd import mesh_io
    from oakink2_tamf_amd.launch import process_object_sdf as P
    from oakink2_tamf_amd.metrics import siv

    fx = load_golden("siv_clip_two_objects.npz")
    names = [str(o) for o in fx["obj_names"]]
    assert all(fx["obj_has_lattice"]) and len(names) == 2
    prefix, out_dir = tmp_path / "meshes", tmp_path / "sdf"
    os.makedirs(prefix)
    R = 40
    meshes = {}
    for n in names:
        m = load_golden(f"siv_lattice_{n}.npz")
        mesh_io.write_ply(str(prefix / f"{n}.ply"), m["verts"], m["faces"])
        meshes[n] = mesh_io.read_mesh(str(prefix / f"{n}.ply"))  # float32, as the launcher reads it
    assert P.main([str(prefix), "--out_dir", str(out_dir), "--resolution", str(R), "--out_json", str(tmp_path / "sdf.json")]) == 0
    index = json.load(open(tmp_path / "sdf.json"))
    assert [o["status"] for o in index["objects"]] == ["written"] * 2 and sorted(os.listdir(out_dir)) == sorted(n + ".pkl" for n in names)
    assert all(o["n_surface_points"] == 0 and o["n_inside"] > 0 for o in index["objects"])  # (else sdf > 0 would not be the mask)
    lat_file, lat_mem = [], []
    for n in names:
        d = pickle.load(open(out_dir / f"{n}.pkl", "rb"))
        from oakink2_tamf_amd.meshdist import SDF_FIELDS

        assert tuple(d) == SDF_FIELDS and d["sdf"].shape == (R ** 3,) and d["point"].shape == (R ** 3, 3) and d["resolution"] == R
        lat_file.append(siv.load_sdf_pickle(str(out_dir / f"{n}.pkl")))  # what compute_score_siv --data.obj_sdf_prefix reads
        lat_mem.append(siv.object_lattice(*meshes[n], resolution=R))
        assert np.array_equal(lat_file[-1].points_in, lat_mem[-1].points_in) and lat_file[-1].el_vol == lat_mem[-1].el_vol
    n = int(fx["avai_len"])
    a = siv.clip_siv(fx["hand_verts_gt"], fx["hand_verts_refined"], fx["faces"], fx["obj_traj"], lat_file, n)
    b = siv.clip_siv(fx["hand_verts_gt"], fx["hand_verts_refined"], fx["faces"], fx["obj_traj"], lat_mem, n)
    assert a == b and max(a[0]) > 0.0
    # an existing file is kept, --overwrite replaces it
    capsys.readouterr()
    assert P.main([str(prefix), "--out_dir", str(out_dir), "--resolution", str(R), "--obj_ids", names[0]]) == 0
    assert "kept" in capsys.readouterr().out
    before = open(out_dir / f"{names[0]}.pkl", "rb").read()
    assert P.main([str(prefix), "--out_dir", str(out_dir), "--resolution", str(R), "--obj_ids", names[0], "--overwrite"]) == 0
    assert open(out_dir / f"{names[0]}.pkl", "rb").read() == before  # the same mesh gives the same bytes


def _parent_render_clip(item, hands, faces, cfg, device):
    """render_samples.render_clip as it was before the penetration map, through the existing API (no vertex colours, no contact map)"""
    from oakink2_tamf_amd import render as R
    from oakink2_tamf_amd.launch import render_samples as RS

    r, d = cfg["render"], cfg["display"]
    frames = RS.drawn_frames(item["len"], r["every"])
    poses = [R.tslrot6d_to_matrix(np.asarray(item["obj_traj"])[k]) for k in range(len(item["obj_list"]))]
    shapes = [np.asarray(item["obj_verts"][k], np.float64) for k in range(len(item["obj_list"]))]
    seen = [np.asarray(h, np.float64)[frames].reshape(-1, 3) for h, _ in hands]
    for m, s in zip(poses, shapes):
        seen.append((np.einsum("fij,pj->fpi", m[frames][:, :, :3], s) + m[frames][:, None, :, 3]).reshape(-1, 3))
    cam = R.look_at_camera(np.concatenate(seen), r["width"], r["height"])
    panels = []
    for verts, colour in hands:
        rd = R.HipRenderer(r["width"], r["height"], device)
        rd.add_mesh(np.asarray(verts, np.float32)[frames], faces, color=colour, smooth=True, name="hand", vertex_colors=None)
        for k, (m, s) in enumerate(zip(poses, shapes)):
            rd.add_mesh(s, item["obj_faces"][k], color=RS.OBJ_COLORS[k % len(RS.OBJ_COLORS)], pose=m[frames], name=str(item["obj_list"][k]), alpha=d["obj_alpha"])
        panels.append(rd.render(cam, layers=d["layers"], ssaa=d["ssaa"])[0].cpu().numpy())
    return frames, np.concatenate(panels, axis=2)


def test_penetration_map(tmp_path, monkeypatch):
    import torch

    import fake_mano
    import test_render_launch_gpu as RL

    from oakink2_tamf_amd import render as R
    from oakink2_tamf_amd.geometry import mesh_contains
    from oakink2_tamf_amd.launch import _score_common as C
    from oakink2_tamf_amd.launch import formats
    from oakink2_tamf_amd.launch import render_samples as RS
    from oakink2_tamf_amd.metrics import pd as PD
    from oakink2_tamf_amd.metrics import siv
    from oracle.fixtures import synthetic_object_mesh

    # the existing render launch test's scene, with the first object of every clip moved INTO the hand (x in [0.04, 0.14] of its wrist)
    monkeypatch.setattr(RL, "OBJ_SHIFT", ((0.09, 0.0, 0.0), (0.30, 0.0, 0.0)))
    paths, cache, tree = RL._tree(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    data = ["--data.cache_dict_filepath", paths["cache"], "--data.obj_embedding_prefix", paths["emb"], "--data.obj_pointcloud_prefix", paths["pc"],
            "--debug.sample_refine_filepath", tree, "--render.width", "64", "--render.height", "64", "--data.obj_model_loader",
            "oracle.fixtures:synthetic_object_mesh", "--with_gt", "--mano.factory", "fake_mano:make", "--render.every", "6"]
    assert RS.main(data + ["--out_dir", str(tmp_path / "plain"), "--out_json", str(tmp_path / "plain.json")]) == 0
    assert RS.main(data + ["--render.penetration_map", "--out_dir", str(tmp_path / "pen"), "--out_json", str(tmp_path / "pen.json")]) == 0
    plain, pen = json.load(open(tmp_path / "plain.json")), json.load(open(tmp_path / "pen.json"))
    assert "penetration" not in plain and pen["penetration"] == {"far_mm": 10.0} and "display" not in pen
    assert {k: v for k, v in pen.items() if k not in ("penetration", "out_dir", "clips")} == {k: v for k, v in plain.items() if k not in ("out_dir", "clips")}

    dev = torch.device("cuda:0")
    cfg = RS.parse_args(data)
    pairs = C.load_pairs(cfg, obj_model_loader=synthetic_object_mesh)
    mano = fake_mano.make(None, dev)
    gts = C.ground_truth_mano([p[0] for p in pairs], mano, dev, 64)[1]
    differs = 0
    for (item, path), gt, clip_plain, clip_pen in zip(pairs, gts, plain["clips"], pen["clips"]):
        save = formats.read_refine_sample(path)
        hands = [(np.asarray(save["verts"], np.float32), RS.HAND_COLOR), (gt, RS.GT_HAND_COLOR)]
        # without the flag: byte for byte what the existing API renders
        frames, images = _parent_render_clip(item, hands, np.asarray(save["faces"]), cfg, dev)
        assert clip_plain["frames"] == frames == clip_pen["frames"]
        for k, fr in enumerate(frames):
            R.write_png(str(tmp_path / "want.png"), images[k])
            name = "frame_%04d.png" % fr
            assert open(os.path.join(clip_plain["dir"], name), "rb").read() == open(tmp_path / "want.png", "rb").read(), (item["info"], fr)
            differs += open(os.path.join(clip_pen["dir"], name), "rb").read() != open(os.path.join(clip_plain["dir"], name), "rb").read()
        # with it: the vertex colours are penetration_colors of the restated depths
        got = RS.penetration_maps(item, hands, frames, 10.0, dev)
        inv = PD.inverse_transf(siv.tslrot6d_to_transf(np.asarray(item["obj_traj"]))).astype(np.float64)
        any_inside = False
        for p, (verts, colour) in enumerate(hands):
            depth = np.zeros((len(frames), verts.shape[1]))
            inside = np.zeros(depth.shape, bool)
            for s, fr in enumerate(frames):
                for k in range(len(item["obj_list"])):
                    ov, of = item["obj_verts"][k], item["obj_faces"][k]
                    q = MR.query_points(np.asarray(verts, np.float32)[fr], inv[k, fr])
                    d = MR.mesh_distance(ov, of, q)[0]
                    m = mesh_contains(ov, of, torch.from_numpy(q).cuda()).cpu().numpy()
                    depth[s] = np.maximum(depth[s], np.where(m, d, 0.0))
                    inside[s] |= m
            # (on the device the launcher computes on: a float32 division by a scalar is not the same instruction everywhere)
            want = R.penetration_colors(torch.from_numpy(depth).to(dev), torch.from_numpy(inside).to(dev), colour, hot=RS.PENETRATION_COLOR, far=0.01)
            assert got[p].shape == (len(frames), verts.shape[1], 3) and got[p].is_cuda and torch.equal(got[p], want), (item["info"], p)
            base = torch.tensor(colour, dtype=torch.float32)
            assert torch.equal(want.cpu()[~torch.from_numpy(inside)], base.expand(int((~inside).sum()), 3))
            host = R.penetration_colors(depth, inside, colour, hot=RS.PENETRATION_COLOR, far=0.01)  # the numpy path: the same to float32 rounding
            assert np.abs(host - want.cpu().numpy()).max() <= 4 * 2.0 ** -24
            any_inside |= bool(inside.any())
        assert any_inside, item["info"]
    assert differs > 0  # the map shows in the pictures
