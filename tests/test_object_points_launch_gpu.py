"""GPU: launch/sample_object_points.py end to end on mesh files the test writes (both directory layouts, three formats), the files it
leaves and what reads them (the dataset, embed_objects), and `--data.obj_mesh_prefix` on embed_objects, compute_score_siv and
render_samples against the same run through an equivalent `--data.obj_model_loader` hook (tests/object_mesh_hook.py)."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import surface_restatement as SR  # noqa: E402

pytestmark = pytest.mark.gpu


def _prefix(root):
    """three objects: sphere.obj, box/scan.stl, tet.ply -> {obj_id: (verts, faces) as read_mesh returns them}"""
    from oakink2_tamf_amd import mesh_io

    os.makedirs(os.path.join(root, "box"))
    mesh_io.write_obj(os.path.join(root, "sphere.obj"), *SR.icosphere(2))
    mesh_io.write_stl(os.path.join(root, "box", "scan.stl"), *SR.cube())
    open(os.path.join(root, "box", "readme.txt"), "w").write("not a mesh")
    mesh_io.write_ply(os.path.join(root, "tet.ply"), *SR.tetrahedron())
    load = mesh_io.directory_loader(root)
    return {oid: load(oid) for oid in ("box", "sphere", "tet")}


def _on_their_faces(point, face_index, verts, faces):
    """the smallest barycentric weight of every point in its face_index triangle, and its distance to that triangle's plane"""
    tri = verts.astype(np.float64)[faces[face_index]]
    e1, e2, d = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], point.astype(np.float64) - tri[:, 0]
    n = np.cross(e1, e2)
    nn = (n * n).sum(1)
    w1 = (np.cross(d, e2) * n).sum(1) / nn
    w2 = (np.cross(e1, d) * n).sum(1) / nn
    return np.minimum(np.minimum(w1, w2), 1.0 - w1 - w2), np.abs((d * n).sum(1)) / np.sqrt(nn)


def test_launcher_writes_reproducible_clouds(tmp_path, capsys):
    from oakink2_tamf_amd.dataset.interaction_segment import InteractionSegmentData
    from oakink2_tamf_amd.launch import sample_object_points as L
    from oakink2_tamf_amd.surface import object_key

    prefix, out = str(tmp_path / "mesh"), str(tmp_path / "pc")
    meshes = _prefix(prefix)
    # --dry_run: the reports, and nothing else happens (no output directory, no library loaded by this call)
    assert L.main([prefix, "--out_dir", out, "--n_points", "256", "--dry_run"]) == 0
    listed = json.loads(capsys.readouterr().out)
    assert [o["obj_id"] for o in listed["objects"]] == ["box", "sphere", "tet"] and not os.path.exists(out)
    assert [(o["n_faces"], o["closed"]) for o in listed["objects"]] == [(12, True), (320, True), (4, True)]
    assert listed["objects"][0]["source"].endswith(os.path.join("box", "scan.stl"))

    assert L.main([prefix, "--out_dir", out, "--n_points", "256", "--seed", "3", "--out_json", str(tmp_path / "index.json")]) == 0
    index = json.load(open(tmp_path / "index.json"))
    assert [(o["obj_id"], o["status"], o["n_points"], o["n_candidates"], o["closed"]) for o in index["objects"]] == \
        [("box", "written", 256, 1024, True), ("sphere", "written", 256, 1024, True), ("tet", "written", 256, 1024, True)]
    assert abs(index["objects"][0]["area"] - 6 * 0.1 ** 2) < 1e-6
    data = {}
    for oid, (v, f) in meshes.items():
        with np.load(os.path.join(out, oid + ".npz")) as z:
            assert sorted(z.files) == ["face_index", "n_candidates", "point", "seed"]
            d = data[oid] = {k: z[k] for k in z.files}
        assert d["point"].dtype == np.float32 and d["point"].shape == (256, 3) and d["face_index"].dtype == np.int64 and d["face_index"].shape == (256,)
        assert d["seed"].dtype == np.uint64 and int(d["seed"]) == 3 and d["n_candidates"].dtype == np.int64 and int(d["n_candidates"]) == 1024
        w, dist = _on_their_faces(d["point"], d["face_index"], v, f)
        assert w.min() >= -1e-6 and dist.max() <= 2.0 ** -23 * np.abs(v).max() * 2, oid
        # the restatement's cloud: samples under the id's key, thinned by the host FPS
        idx, ref = SR.point_cloud(v, f, 256, 4, 3, object_key(oid))
        assert ref["near"].sum() == 0 and np.array_equal(d["face_index"], ref["face"][idx])
        assert np.array_equal(d["point"].view(np.uint32), ref["point"][idx].view(np.uint32))
    # what the dataset reads
    ds = InteractionSegmentData.__new__(InteractionSegmentData)
    ds.interaction_object_list, ds.obj_pointcloud_prefix = ["box", "sphere", "tet"], out
    store = ds.load_object_pointcloud()
    assert all(np.array_equal(store[o], data[o]["point"]) for o in data)

    # a rerun keeps the files; --overwrite reproduces them byte for byte
    raw = {o: open(os.path.join(out, o + ".npz"), "rb").read() for o in data}
    stamp = {o: os.stat(os.path.join(out, o + ".npz")).st_mtime_ns for o in data}
    capsys.readouterr()
    assert L.main([prefix, "--out_dir", out, "--n_points", "256", "--seed", "4"]) == 0
    assert capsys.readouterr().out.count("kept") == 3
    assert all(os.stat(os.path.join(out, o + ".npz")).st_mtime_ns == stamp[o] for o in data)
    assert L.main([prefix, "--out_dir", out, "--n_points", "256", "--seed", "3", "--overwrite"]) == 0
    assert all(open(os.path.join(out, o + ".npz"), "rb").read() == raw[o] for o in data)
    assert all(os.stat(os.path.join(out, o + ".npz")).st_mtime_ns != stamp[o] for o in data)
    # another seed, or the same mesh under another id (another key), is another cloud
    other = str(tmp_path / "pc_seed4")
    assert L.main([prefix, "--out_dir", other, "--n_points", "256", "--seed", "4", "--obj_ids", "tet"]) == 0
    assert sorted(os.listdir(other)) == ["tet.npz"]
    assert not np.array_equal(np.load(os.path.join(other, "tet.npz"))["point"], data["tet"]["point"])

    # --scale 0.001 --with_normals: the cloud of the scaled mesh, xyz | normal
    mm = str(tmp_path / "pc_mm")
    assert L.main([prefix, "--out_dir", mm, "--n_points", "256", "--seed", "3", "--scale", "0.001", "--with_normals", "--obj_ids", "sphere,box"]) == 0
    for oid in ("sphere", "box"):
        v, f = meshes[oid]
        vs = (v.astype(np.float64) * 0.001).astype(np.float32)
        with np.load(os.path.join(mm, oid + ".npz")) as z:
            p, fi = z["point"], z["face_index"]
        assert p.shape == (256, 6) and p.dtype == np.float32
        w, dist = _on_their_faces(p[:, :3], fi, vs, f)
        assert w.min() >= -1e-6 and dist.max() <= 2.0 ** -22 * np.abs(vs).max()
        assert np.abs(p[:, :3]).max() <= np.abs(vs).max() and np.abs(p[:, :3]).max() > 0.5 * np.abs(vs).max()
        n = np.cross(vs[f[fi, 1]].astype(np.float64) - vs[f[fi, 0]], vs[f[fi, 2]].astype(np.float64) - vs[f[fi, 0]])
        assert np.abs(p[:, 3:] - n / np.linalg.norm(n, axis=1, keepdims=True)).max() <= 2.0 ** -22

    # refusals name what is wrong
    for argv, word in (([prefix, "--out_dir", out, "--n_points", "8192", "--oversample", "5"], "32768"), ([prefix, "--obj_ids", "nothing"], "no file under"),
                       ([str(tmp_path / "absent")], "no directory")):
        with pytest.raises(SystemExit) as e:
            L.main(argv)
        assert word in str(e.value), argv


def test_launcher_at_the_default_size_and_from_points(tmp_path):
    from oakink2_tamf_amd.launch import sample_object_points as L

    prefix, out = str(tmp_path / "mesh"), str(tmp_path / "pc")
    meshes = _prefix(prefix)
    assert L.main([prefix, "--out_dir", out, "--obj_ids", "sphere"]) == 0  # 8192 of 32768
    v, f = meshes["sphere"]
    with np.load(os.path.join(out, "sphere.npz")) as z:
        p, fi = z["point"], z["face_index"]
        assert p.shape == (8192, 3) and int(z["n_candidates"]) == 32768 and int(z["seed"]) == 0
    w, dist = _on_their_faces(p, fi, v, f)
    assert w.min() >= -1e-6 and dist.max() <= 2.0 ** -22 * np.abs(v).max()
    assert len(np.unique(fi)) == 320  # every face of the sphere carries some of the 8192 points
    # --from_points: the written cloud as a scan of 8192 points, thinned to 512
    scans = str(tmp_path / "scan")
    os.makedirs(scans)
    np.save(os.path.join(scans, "sphere.npy"), p)
    assert L.main([scans, "--from_points", "--out_dir", str(tmp_path / "pc2"), "--n_points", "512"]) == 0
    with np.load(str(tmp_path / "pc2" / "sphere.npz")) as z:
        assert sorted(z.files) == ["n_candidates", "point", "point_index", "seed"] and int(z["n_candidates"]) == 8192
        assert np.array_equal(z["point"], p[z["point_index"]]) and z["point"].shape == (512, 3) and z["point_index"][0] == 0


def test_embed_objects_from_meshes_equals_embed_objects_from_the_written_files(tmp_path):
    import torch
    import yaml

    import pointenc_fixture as PF

    from oakink2_tamf_amd.launch import embed_objects as E
    from oakink2_tamf_amd.launch import sample_object_points as L
    from oakink2_tamf_amd.model.point_encoder import PREFIX

    cfg = dict(PF.CASES["tiny"][0])  # point_dims 3, 17 groups of 8
    sd = PF.seeded_state_dict(cfg, PF.WEIGHT_SEED["tiny"])
    ckpt, cfg_path = str(tmp_path / "enc.pt"), str(tmp_path / "enc.yml")
    torch.save({"state_dict": {PREFIX + k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}, ckpt)
    with open(cfg_path, "w") as f:
        yaml.safe_dump({"npoints": 256, "model": cfg}, f)
    prefix, pc = str(tmp_path / "mesh"), str(tmp_path / "pc")
    _prefix(prefix)
    assert L.main([prefix, "--out_dir", pc, "--n_points", "256", "--seed", "7"]) == 0
    common = ["--point_encoder.ckpt", ckpt, "--point_encoder.cfg", cfg_path]
    assert E.main(common + ["--data.obj_pointcloud_prefix", pc, "--out_dir", str(tmp_path / "from_npz")]) == 0
    assert E.main(common + ["--data.obj_mesh_prefix", prefix, "--sample.seed", "7", "--out_dir", str(tmp_path / "from_mesh")]) == 0
    assert E.main(common + ["--data.obj_mesh_prefix", prefix, "--sample.seed", "8", "--out_dir", str(tmp_path / "seed8"), "--obj_ids", "box"]) == 0
    for oid in ("box", "sphere", "tet"):
        a = torch.load(str(tmp_path / "from_npz" / f"{oid}.pt"), weights_only=True)
        b = torch.load(str(tmp_path / "from_mesh" / f"{oid}.pt"), weights_only=True)
        assert a.shape == (256,) and a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32)), oid
    assert not torch.equal(torch.load(str(tmp_path / "seed8" / "box.pt"), weights_only=True), torch.load(str(tmp_path / "from_npz" / "box.pt"), weights_only=True))


def test_score_siv_with_a_mesh_prefix_equals_the_hook(tmp_path, monkeypatch):
    import object_mesh_hook
    import test_score_cpu as S

    from oakink2_tamf_amd.launch import compute_score_siv as L

    paths, cache, tree = S._synthetic_tree(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    obj_ids = sorted({o for traj in cache["interaction_segment_obj_traj_list"] for o in traj})
    object_mesh_hook.write_prefix(str(tmp_path / "mesh"), obj_ids)
    used = sorted({o for i in (0, 1, 2) for o in cache["interaction_segment_obj_traj_list"][i]})
    object_mesh_hook.write_prefix(str(tmp_path / "mesh_open"), obj_ids, open_ids=used[:1])
    data = ["--data.cache_dict_filepath", paths["cache"], "--data.obj_embedding_prefix", paths["emb"], "--data.obj_pointcloud_prefix", paths["pc"],
            "--debug.sample_refine_filepath", tree, "--mano.factory", "fake_mano:make"]
    with pytest.raises(SystemExit) as e:  # both sources of meshes: refused by the parser
        L.main(data + ["--data.obj_mesh_prefix", str(tmp_path / "mesh"), "--data.obj_model_loader", "object_mesh_hook:load_obj"])
    assert e.value.code == 2
    assert L.main(data + ["--data.obj_model_loader", "object_mesh_hook:load_obj", "--out_json", str(tmp_path / "hook.json")]) == 0
    assert L.main(data + ["--data.obj_mesh_prefix", str(tmp_path / "mesh"), "--out_json", str(tmp_path / "prefix.json")]) == 0
    hook, pre = json.load(open(tmp_path / "hook.json")), json.load(open(tmp_path / "prefix.json"))
    assert "n_objects_open" not in hook and pre.pop("n_objects_open") == 0 and pre.pop("objects_open") == []
    assert pre == hook and hook["n_objects_skipped"] == 0 and hook["n_frames"] > 0
    assert L.main(data + ["--data.obj_mesh_prefix", str(tmp_path / "mesh_open"), "--out_json", str(tmp_path / "open.json")]) == 0
    res = json.load(open(tmp_path / "open.json"))
    assert res["n_objects_open"] == 1 and res["objects_open"] == used[:1] and res["n_frames"] == hook["n_frames"]


def test_render_samples_with_a_mesh_prefix_equals_the_hook(tmp_path, monkeypatch):
    import object_mesh_hook
    import test_render_launch_gpu as R

    from oakink2_tamf_amd.launch import render_samples as L

    paths, cache, tree = R._tree(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    object_mesh_hook.write_prefix(str(tmp_path / "mesh"), sorted({o for traj in cache["interaction_segment_obj_traj_list"] for o in traj}))
    data = ["--data.cache_dict_filepath", paths["cache"], "--data.obj_embedding_prefix", paths["emb"], "--data.obj_pointcloud_prefix", paths["pc"],
            "--debug.sample_refine_filepath", tree, "--render.width", "64", "--render.height", "64", "--render.every", "5"]
    with pytest.raises(SystemExit) as e:
        L.main(data + ["--data.obj_mesh_prefix", str(tmp_path / "mesh"), "--data.obj_model_loader", "object_mesh_hook:load_obj", "--out_dir", str(tmp_path / "no")])
    assert e.value.code == 2 and not (tmp_path / "no").exists()
    assert L.main(data + ["--data.obj_model_loader", "object_mesh_hook:load_obj", "--out_dir", str(tmp_path / "hook"), "--out_json", str(tmp_path / "hook.json")]) == 0
    assert L.main(data + ["--data.obj_mesh_prefix", str(tmp_path / "mesh"), "--out_dir", str(tmp_path / "prefix"), "--out_json", str(tmp_path / "prefix.json")]) == 0

    def files(root):
        return {os.path.relpath(os.path.join(d, n), root): open(os.path.join(d, n), "rb").read() for d, _, names in os.walk(root) for n in names}

    a, b = files(str(tmp_path / "hook")), files(str(tmp_path / "prefix"))
    assert sorted(a) == sorted(b) and len(a) >= 2 * (4 + 1) and all(n.endswith(".png") for n in a)
    assert all(a[n] == b[n] for n in a)
    ja, jb = open(tmp_path / "hook.json").read(), open(tmp_path / "prefix.json").read()
    assert ja.replace(str(tmp_path / "hook"), "OUT") == jb.replace(str(tmp_path / "prefix"), "OUT")
    assert all(c["objects"] == "mesh" for c in json.loads(ja)["clips"])
