"""The launchers around the point-to-mesh distance without a GPU: compute_score_pd's arguments, --dry_run and refusals, the scripts'
-n, process_object_sdf --dry_run, and render_samples' --render.penetration_map flags and refusals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")) if p not in sys.path]

import object_mesh_hook  # noqa: E402
import test_score_cpu as S  # noqa: E402


def test_pd_dry_run_lists_the_pairs_and_takes_sivs_argument_names(tmp_path):
    from oakink2_tamf_amd.launch import compute_score_pd, compute_score_siv

    paths, cache, tree = S._synthetic_tree(str(tmp_path))
    r = S._launch("compute_score_pd", S._data_args(paths, tree) + ["--data.obj_model_loader", "object_mesh_hook:load_obj", "--dry_run"], str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    infos = cache["interaction_segment_info_list"]
    assert out["n_clips"] == 3 and [tuple(p["info"]) for p in out["pairs"]] == [tuple(infos[i]) for i in (0, 1, 2)]
    assert out["stride"] == 20 and out["obj_model_loader"] == "object_mesh_hook:load_obj" and "obj_mesh_prefix" not in out
    argv = S._data_args(paths, tree) + ["--data.obj_model_loader", "m:f", "--mano.factory", "fake_mano:make", "--save_dir", "o", "--out_json", "j",
                                        "--batch_size", "8", "--device", "cuda:1"]
    a, b = compute_score_pd.parse_args(argv), compute_score_siv.parse_args(argv)
    assert a["runtime"].pop("stride") == 20 and b["data"].pop("obj_sdf_prefix") is None and a == b
    assert compute_score_pd.parse_args(argv + ["--stride", "7"])["runtime"]["stride"] == 7


def _refused(parse, argv, capsys):
    """argparse's refusal of `argv`, in this process: exit status 2 -> what it wrote to stderr"""
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        parse(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_pd_refusals(tmp_path, capsys):
    from oakink2_tamf_amd.launch import compute_score_pd as L

    paths, _, tree = S._synthetic_tree(str(tmp_path))
    args = S._data_args(paths, tree)
    assert "the PD score needs the objects' meshes" in _refused(L.parse_args, args + ["--dry_run"], capsys)
    assert "give one" in _refused(L.parse_args, args + ["--data.obj_model_loader", "a:b", "--data.obj_mesh_prefix", str(tmp_path), "--dry_run"], capsys)
    assert "--stride" in _refused(L.parse_args, args + ["--data.obj_model_loader", "a:b", "--stride", "0", "--dry_run"], capsys)
    assert "unrecognized" in _refused(L.parse_args, args + ["--data.obj_model_loader", "a:b", "--no_such_flag", "1"], capsys)
    r = S._launch("compute_score_pd", args + ["--data.obj_model_loader", "object_mesh_hook:load_obj"], str(tmp_path))  # the launcher itself, once
    assert r.returncode != 0 and "the refine stage needs MANO: pass --mano.factory module:function" in r.stderr


def test_scripts_print_their_command():
    r = subprocess.run(["bash", os.path.join(ROOT, "script", "compute_score_pd.sh"), "-n", "test", "arch_mdm_l__0399", "--stride", "10"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("python -m oakink2_tamf_amd.launch.compute_score_pd ") and last.endswith("--stride 10")
    assert "common/sample_refine/main/sample/test/arch_mdm_l__0399" in last and "common/save_cache_dict/main/cache/test.pkl" in last
    assert subprocess.run(["bash", os.path.join(ROOT, "script", "compute_score_pd.sh"), "-n", "test"], capture_output=True).returncode == 2
    r = subprocess.run(["bash", os.path.join(ROOT, "script", "process_object_sdf.sh"), "-n", "meshes dir", "--resolution", "64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == "python -m oakink2_tamf_amd.launch.process_object_sdf meshes\\ dir --resolution 64"
    assert subprocess.run(["bash", os.path.join(ROOT, "script", "process_object_sdf.sh"), "-n"], capture_output=True).returncode == 2
    for name in ("compute_score_pd.sh", "process_object_sdf.sh"):
        assert os.access(os.path.join(ROOT, "script", name), os.X_OK)


def test_process_object_sdf_dry_run_and_selection(tmp_path, capsys):
    prefix = str(tmp_path / "meshes")
    ids = ["O02@0001@00001", "O02@0002@00001", "O02@0003@00001"]
    object_mesh_hook.write_prefix(prefix, ids, open_ids=(ids[1],))
    r = S._launch("process_object_sdf", [prefix, "--dry_run", "--out_dir", str(tmp_path / "sdf"), "--resolution", "32"], str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout)
    assert out["resolution"] == 32 and out["bbox_expand_ratio"] == 1.2 and [o["obj_id"] for o in out["objects"]] == ids
    assert [o["closed"] for o in out["objects"]] == [True, False, True] and out["objects"][0]["sdf"] == str(tmp_path / "sdf" / (ids[0] + ".pkl"))
    assert not os.path.exists(tmp_path / "sdf")
    from oakink2_tamf_amd.launch import process_object_sdf as P

    capsys.readouterr()
    assert P.main([prefix, "--dry_run", "--obj_ids", ids[2]]) == 0
    assert [o["obj_id"] for o in json.loads(capsys.readouterr().out)["objects"]] == [ids[2]]
    for argv, msg in (([prefix, "--dry_run", "--obj_ids", "nope"], "nope"), ([prefix, "--dry_run", "--resolution", "513"], "--resolution"),
                      ([str(tmp_path / "none"), "--dry_run"], "is no directory")):
        with pytest.raises(SystemExit) as e:
            P.main(argv)
        assert msg in str(e.value.code), argv


def test_penetration_map_flags_and_refusals(tmp_path, capsys):
    from oakink2_tamf_amd.launch import render_samples as RS

    paths, _, tree = S._synthetic_tree(str(tmp_path))
    args = S._data_args(paths, tree)
    plain = RS.parse_args(args + ["--data.obj_model_loader", "a:b"])
    assert "penetration" not in plain and plain["display"] == RS.DISPLAY_DEFAULTS  # without the flag the run is configured as before
    cfg = RS.parse_args(args + ["--data.obj_model_loader", "a:b", "--render.penetration_map"])
    assert cfg["penetration"] == {"far_mm": 10.0} and cfg["display"] == RS.DISPLAY_DEFAULTS
    assert {k: v for k, v in cfg.items() if k != "penetration"} == plain
    assert RS.parse_args(args + ["--data.obj_mesh_prefix", str(tmp_path), "--render.penetration_map", "--render.penetration_far_mm", "25"])["penetration"] == {"far_mm": 25.0}
    for extra, msg in ((["--render.penetration_map"], "measures the hand against the objects' meshes"),
                       (["--data.obj_model_loader", "a:b", "--render.penetration_map", "--render.contact_map"], "both colour the hand"),
                       (["--data.obj_model_loader", "a:b", "--render.penetration_far_mm", "5"], "belongs to --render.penetration_map"),
                       (["--data.obj_model_loader", "a:b", "--render.penetration_map", "--render.penetration_far_mm", "0"], "positive")):
        assert msg in _refused(RS.parse_args, args + extra + ["--dry_run"], capsys), extra
    r = S._launch("render_samples", args + ["--data.obj_model_loader", "object_mesh_hook:load_obj", "--render.penetration_map", "--dry_run"], str(tmp_path))
    assert r.returncode == 0 and json.loads(r.stdout.strip().splitlines()[-1])["penetration"] == {"far_mm": 10.0}
    capsys.readouterr()
    assert RS.main(args + ["--data.obj_model_loader", "object_mesh_hook:load_obj", "--dry_run"]) == 0
    assert "penetration" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
