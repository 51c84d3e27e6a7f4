"""The launchers' winding-number sign without a GPU: the flags, what a run without them is configured as (exactly as before), the dry
runs' report of the sign, and the refusals."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")) if p not in sys.path]

import object_mesh_hook  # noqa: E402
import test_score_cpu as S  # noqa: E402
from test_pd_launch_cpu import _refused  # noqa: E402


def test_pd_sign_flag(tmp_path, capsys):
    from oakink2_tamf_amd.launch import compute_score_pd as L

    paths, _, tree = S._synthetic_tree(str(tmp_path))
    args = S._data_args(paths, tree) + ["--data.obj_model_loader", "object_mesh_hook:load_obj"]
    plain = L.parse_args(args)
    assert "sign" not in plain["runtime"]  # without the flag the run is configured as before
    cfg = L.parse_args(args + ["--sign", "winding"])
    assert cfg["runtime"].pop("sign") == "winding" and cfg == plain
    assert L.parse_args(args + ["--sign", "parity"])["runtime"]["sign"] == "parity"
    assert "invalid choice" in _refused(L.parse_args, args + ["--sign", "pysdf"], capsys)
    for extra, want in (([], "parity"), (["--sign", "winding"], "winding")):
        capsys.readouterr()
        assert L.main(args + extra + ["--dry_run"]) == 0
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["sign"] == want


def test_siv_obj_sign_flag(tmp_path, capsys):
    from oakink2_tamf_amd.launch import compute_score_siv as L

    paths, _, tree = S._synthetic_tree(str(tmp_path))
    args = S._data_args(paths, tree) + ["--data.obj_model_loader", "object_mesh_hook:load_obj"]
    plain = L.parse_args(args)
    assert "obj_sign" not in plain["data"]
    cfg = L.parse_args(args + ["--data.obj_sign", "winding"])
    assert cfg["data"].pop("obj_sign") == "winding" and cfg == plain
    assert "invalid choice" in _refused(L.parse_args, args + ["--data.obj_sign", "both"], capsys)
    for extra, want in (([], "parity"), (["--data.obj_sign", "winding"], "winding")):
        capsys.readouterr()
        assert L.main(args + extra + ["--dry_run"]) == 0
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["obj_sign"] == want


def test_process_object_sdf_sign_flag(tmp_path, capsys):
    from oakink2_tamf_amd.launch import process_object_sdf as P

    prefix = str(tmp_path / "meshes")
    ids = ["O02@0001@00001", "O02@0002@00001"]
    object_mesh_hook.write_prefix(prefix, ids, open_ids=(ids[1],))
    assert P.make_parser().parse_args([prefix]).sign == "parity"
    for extra, want in (([], "parity"), (["--sign", "winding"], "winding")):
        capsys.readouterr()
        assert P.main([prefix, "--dry_run"] + extra) == 0
        out = json.loads(capsys.readouterr().out)
        assert out["sign"] == want and [o["closed"] for o in out["objects"]] == [True, False]
    with pytest.raises(SystemExit) as e:
        P.main([prefix, "--dry_run", "--sign", "pysdf"])
    assert e.value.code == 2


def test_render_penetration_sign_flag_and_refusals(tmp_path, capsys):
    from oakink2_tamf_amd.launch import render_samples as RS

    paths, _, tree = S._synthetic_tree(str(tmp_path))
    args = S._data_args(paths, tree) + ["--data.obj_model_loader", "a:b"]
    pen = RS.parse_args(args + ["--render.penetration_map"])
    assert pen["penetration"] == {"far_mm": 10.0}  # without the new flag: as before
    cfg = RS.parse_args(args + ["--render.penetration_map", "--render.penetration_sign", "winding"])
    assert cfg["penetration"] == {"far_mm": 10.0, "sign": "winding"}
    assert {k: v for k, v in cfg.items() if k != "penetration"} == {k: v for k, v in pen.items() if k != "penetration"}
    assert RS.parse_args(args + ["--render.penetration_map", "--render.penetration_sign", "parity"])["penetration"]["sign"] == "parity"
    assert "belongs to --render.penetration_map" in _refused(RS.parse_args, args + ["--render.penetration_sign", "winding", "--dry_run"], capsys)
    assert "invalid choice" in _refused(RS.parse_args, args + ["--render.penetration_map", "--render.penetration_sign", "x"], capsys)
    capsys.readouterr()
    assert RS.main(S._data_args(paths, tree) + ["--data.obj_model_loader", "object_mesh_hook:load_obj", "--render.penetration_map",
                                                 "--render.penetration_sign", "winding", "--dry_run"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["penetration"] == {"far_mm": 10.0, "sign": "winding"}


def test_library_functions_refuse_an_unknown_sign():
    import numpy as np

    from oakink2_tamf_amd import meshdist
    from oakink2_tamf_amd.metrics import pd, siv

    v = np.asarray([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    f = np.asarray([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    with pytest.raises(ValueError, match="sign must be"):
        meshdist.process_sdf(v, f, sign="pysdf")
    with pytest.raises(ValueError, match="sign must be"):
        siv.object_lattice(v, f, sign="pysdf")
    hv = np.zeros((4, 5, 3), np.float32)
    with pytest.raises(ValueError, match="sign must be"):
        pd.clip_pd(hv, hv, np.zeros((1, 4, 9), np.float32), None, [None], 4, sign="pysdf")
    with pytest.raises(ValueError, match="needs winding_set"):
        pd.clip_pd(hv, hv, np.zeros((1, 4, 9), np.float32), None, [None], 4, sign="winding")


def test_scripts_pass_the_flags_through():
    for script, tail in (("compute_score_pd.sh", ["test", "arch_mdm_l__0399", "--sign", "winding"]),
                         ("compute_score_siv.sh", ["test", "arch_mdm_l__0399", "--data.obj_sign", "winding"]),
                         ("render_samples.sh", ["test", "arch_mdm_l__0399", "--render.penetration_map", "--render.penetration_sign", "winding"]),
                         ("process_object_sdf.sh", ["meshes", "--sign", "winding"])):
        r = subprocess.run(["bash", os.path.join(ROOT, "script", script), "-n"] + tail, capture_output=True, text=True)
        assert r.returncode == 0, (script, r.stderr)
        assert r.stdout.strip().splitlines()[-1].endswith(" ".join(tail[-2:])), (script, r.stdout)
