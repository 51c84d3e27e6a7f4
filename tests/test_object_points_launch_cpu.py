"""The CPU half of the object point-cloud launchers: launch/sample_object_points.py's work list, dry run, refusals and its
time-independent .npz writer, script/sample_object_points.sh, and `--data.obj_mesh_prefix` as compute_score_siv, render_samples and
embed_objects parse it.  No GPU."""
import json
import os
import shlex
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")) if p not in sys.path]

import surface_restatement as SR  # noqa: E402
from oakink2_tamf_amd import mesh_io  # noqa: E402


def _prefix(root):
    os.makedirs(os.path.join(root, "box"))
    mesh_io.write_obj(os.path.join(root, "sphere.obj"), *SR.icosphere(1))
    v, f = SR.cube()
    mesh_io.write_stl(os.path.join(root, "box", "scan.stl"), v, f[1:])  # an open box
    mesh_io.write_ply(os.path.join(root, "tet.ply"), *SR.tetrahedron())
    return root


def test_dry_run_lists_the_reports_and_touches_nothing(tmp_path, capsys):
    from oakink2_tamf_amd.launch import sample_object_points as L

    prefix = _prefix(str(tmp_path / "mesh"))
    assert L.main([prefix, "--out_dir", str(tmp_path / "pc"), "--dry_run", "--scale", "0.001"]) == 0
    out = json.loads(capsys.readouterr().out)
    assert (out["n_points"], out["oversample"], out["seed"], out["scale"], out["with_normals"], out["from_points"]) == (8192, 4, 0, 0.001, False, False)
    objs = out["objects"]
    assert [o["obj_id"] for o in objs] == ["box", "sphere", "tet"] and not (tmp_path / "pc").exists()
    assert [(o["n_faces"], o["closed"], o["n_boundary_edges"]) for o in objs] == [(11, False, 3), (80, True, 0), (4, True, 0)]
    assert abs(objs[0]["area"] - 5.5 * 1e-8) < 1e-12  # the open box in metres: 5.5 sides of (0.1 mm)^2
    assert objs[0]["pointcloud"] == str(tmp_path / "pc" / "box.npz")
    assert L.main([prefix, "--obj_ids", "tet,sphere", "--dry_run"]) == 0
    assert [o["obj_id"] for o in json.loads(capsys.readouterr().out)["objects"]] == ["tet", "sphere"]
    ids = tmp_path / "ids.txt"
    ids.write_text("sphere\n")
    assert L.main([prefix, "--obj_ids", f"?(file:{ids})", "--dry_run"]) == 0
    assert [o["obj_id"] for o in json.loads(capsys.readouterr().out)["objects"]] == ["sphere"]


def test_refusals(tmp_path):
    from oakink2_tamf_amd.launch import sample_object_points as L

    prefix = _prefix(str(tmp_path / "mesh"))
    mesh_io.write_obj(os.path.join(prefix, "tet.obj"), *SR.tetrahedron())  # tet.ply and tet.obj
    (tmp_path / "empty").mkdir()
    (tmp_path / "mesh" / "bad.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    for argv, word in (([prefix, "--n_points", "8192", "--oversample", "5", "--dry_run"], "at most 32768"),
                       ([prefix, "--n_points", "0"], "at least 1"), ([prefix, "--scale", "0"], "--scale"), ([prefix, "--seed", "-1"], "--seed"),
                       ([prefix, "--from_points", "--with_normals"], "--with_normals needs a mesh"),
                       ([prefix, "--obj_ids", "tet", "--dry_run"], "2 candidates"), ([prefix, "--obj_ids", "none", "--dry_run"], "no file under"),
                       ([prefix, "--obj_ids", "bad", "--dry_run"], "bad.obj: face 0"), ([str(tmp_path / "absent")], "no directory"),
                       ([str(tmp_path / "empty"), "--dry_run"], "no mesh file under")):
        with pytest.raises(SystemExit) as e:
            L.main(argv)
        assert word in str(e.value), (argv, str(e.value))


def test_written_npz_depends_on_the_arrays_alone(tmp_path):
    from oakink2_tamf_amd.launch import sample_object_points as L

    arrays = {"point": np.arange(12, dtype=np.float32).reshape(4, 3), "face_index": np.arange(4, dtype=np.int64), "seed": np.uint64(2 ** 63 + 5),
              "n_candidates": np.int64(16)}
    a, b = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    L.write_npz(a, arrays)
    os.utime(a, (0, 0))
    L.write_npz(b, arrays)
    assert open(a, "rb").read() == open(b, "rb").read() and not os.path.exists(a + ".tmp")
    with np.load(a, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(arrays) and all(np.array_equal(z[k], arrays[k]) and z[k].dtype == np.asarray(arrays[k]).dtype for k in arrays)
    assert np.array_equal(mesh_io.read_points(a), arrays["point"])
    v = np.array([[1.5, -2.25, 1e-3]], np.float32)
    assert L.scaled(v, 1.0) is v and np.array_equal(L.scaled(v, 0.001), (v.astype(np.float64) * 0.001).astype(np.float32))


def test_shell_entry_point():
    path = os.path.join(ROOT, "script", "sample_object_points.sh")
    assert os.access(path, os.X_OK)
    r = subprocess.run(["bash", path, "-n", "assets/object mesh", "--n_points", "2048", "--scale", "0.001"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "mesh prefix: assets/object mesh" in r.stdout
    toks = shlex.split([l for l in r.stdout.splitlines() if l.startswith("python -m ")][-1])
    assert toks[:3] == ["python", "-m", "oakink2_tamf_amd.launch.sample_object_points"]
    from oakink2_tamf_amd.launch import sample_object_points as L

    a = L.make_parser().parse_args(toks[3:])
    assert (a.prefix, a.n_points, a.scale, a.oversample, a.seed) == ("assets/object mesh", 2048, 0.001, 4, 0)
    assert a.out_dir == os.path.join("common", "retrieve_obj_pointcloud", "main", "pointcloud")
    r = subprocess.run(["bash", path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr
    r = subprocess.run(["bash", path, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "mesh prefix" in r.stdout


@pytest.mark.parametrize("module", ["compute_score_siv", "render_samples"])
def test_mesh_prefix_flag_of_the_consumers(tmp_path, module):
    import importlib

    L = importlib.import_module("oakink2_tamf_amd.launch." + module)
    prefix = _prefix(str(tmp_path / "mesh"))
    d = L.parse_args([])
    assert "obj_mesh_prefix" not in d["data"] and d["data"]["obj_model_loader"] is None  # without the flag: configured as before
    assert L.mesh_loader(d) is None
    hook = L.parse_args(["--data.obj_model_loader", "oracle.fixtures:synthetic_object_mesh"])
    assert "obj_mesh_prefix" not in hook["data"] and L.mesh_loader(hook)("C1")[1].shape[1] == 3
    cfg = L.parse_args(["--data.obj_mesh_prefix", os.path.relpath(prefix)])
    assert cfg["data"]["obj_mesh_prefix"] == prefix and cfg["data"]["obj_model_loader"] is None
    load = L.mesh_loader(cfg)
    v, f = load("box")
    assert v.dtype == np.float32 and f.shape == (11, 3) and load("box")[0] is v
    with pytest.raises(SystemExit, match="'nothing': no file under"):
        load("nothing")
    with pytest.raises(SystemExit) as e:
        L.parse_args(["--data.obj_mesh_prefix", prefix, "--data.obj_model_loader", "oracle.fixtures:synthetic_object_mesh"])
    assert e.value.code == 2
    with pytest.raises(SystemExit, match="no directory"):
        L.mesh_loader(L.parse_args(["--data.obj_mesh_prefix", str(tmp_path / "absent")]))


def test_embed_objects_lists_meshes(tmp_path, capsys):
    from oakink2_tamf_amd.launch import embed_objects as E

    prefix = _prefix(str(tmp_path / "mesh"))
    assert E.main(["--data.obj_mesh_prefix", prefix, "--out_dir", str(tmp_path / "emb"), "--dry_run"]) == 0
    work = json.loads(capsys.readouterr().out)["work"]
    assert [(w["obj_id"], os.path.relpath(w["pointcloud"], prefix)) for w in work] == [("box", os.path.join("box", "scan.stl")), ("sphere", "sphere.obj"), ("tet", "tet.ply")]
    assert work[0]["embedding"] == str(tmp_path / "emb" / "box.pt")
    a = E.make_parser().parse_args([])
    assert a.mesh_prefix is None and (a.sample_oversample, a.sample_seed, a.sample_scale, a.sample_with_normals) == (4, 0, 1.0, False)
