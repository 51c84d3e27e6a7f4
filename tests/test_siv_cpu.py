"""CPU: the SIV evaluation away from the GPU - the host half of object_lattice against the fixtures of tools/capture_siv_golden.py
(exact: the same float64 numpy lines), the pickle reader, the job list of clip_siv, the C header / export lists of libtamf_eval.so and
the launcher's arguments and --dry_run."""
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

LATTICES = ["rotbox", "sphere", "torus", "twoparts", "aabox"]


@pytest.mark.parametrize("name", LATTICES)
def test_lattice_axes_match_the_reference_exactly(name):
    from oakink2_tamf_amd.metrics import siv

    fx = load_golden(f"siv_lattice_{name}.npz")
    R = int(fx["R"])
    ax = siv.lattice_axes(fx["verts"], float(fx["bbox_expand_ratio"]), R)
    for key in ("mesh_center", "extent", "extent_expanded", "tick_unit"):
        assert np.array_equal(ax[key], fx[key]), key
    assert not np.array_equal(ax["tick_unit"], ax["ticks"][1] - ax["ticks"][0])  # the reference's quirk: / R, not / (R - 1)
    assert ax["ticks"].shape == (R, 3)
    # point order: flat index (i * R + j) * R + k, `point` = lattice + centre; the score adds the centre once more
    assert np.array_equal(siv.lattice_points(ax["ticks"], ax["mesh_center"], [0, R ** 3 - 1]),
                          np.stack([fx["point_first"], fx["point_last"]]) + ax["mesh_center"])
    idx = np.array([1, R, R * R, 5 * R * R + 3 * R + 2])
    x, y, z = np.meshgrid(ax["ticks"][:, 0], ax["ticks"][:, 1], ax["ticks"][:, 2], indexing="ij")
    q = np.vstack((x.flatten(), y.flatten(), z.flatten())).T
    assert np.array_equal(siv.lattice_points(ax["ticks"], ax["mesh_center"], idx), (q[idx] + ax["mesh_center"]) + ax["mesh_center"])
    mask = np.unpackbits(fx["mask_packed"])[: R ** 3].astype(bool)
    assert int(mask.sum()) == int(fx["n_inside"]) > 0


def test_load_sdf_pickle_round_trip(tmp_path):
    from oakink2_tamf_amd.metrics import siv

    fx = load_golden("siv_lattice_rotbox.npz")
    R = int(fx["R"])
    ax = siv.lattice_axes(fx["verts"], 1.2, R)
    mask = np.unpackbits(fx["mask_packed"])[: R ** 3].astype(bool)
    x, y, z = np.meshgrid(ax["ticks"][:, 0], ax["ticks"][:, 1], ax["ticks"][:, 2], indexing="ij")
    point = np.vstack((x.flatten(), y.flatten(), z.flatten())).T + ax["mesh_center"]
    d = {"mesh_center": ax["mesh_center"], "bbox": np.zeros((8, 3)), "bbox_centered": np.zeros((8, 3)), "bbox_centered_expanded": np.zeros((8, 3)),
         "bbox_expanded": np.zeros((8, 3)), "bbox_expand_ratio": 1.2, "resolution": R, "extent": ax["extent"],
         "extent_expanded": ax["extent_expanded"], "tick_unit": ax["tick_unit"], "point": point, "sdf": np.where(mask, 0.5, -0.5)}
    path = tmp_path / "obj.pkl"
    with open(path, "wb") as f:
        pickle.dump(d, f)
    lat = siv.load_sdf_pickle(str(path))
    assert lat.ticks is None and lat.resolution == R and lat.el_vol == float(np.prod(ax["tick_unit"]))
    assert np.array_equal(lat.points_in, siv.lattice_points(ax["ticks"], ax["mesh_center"], np.nonzero(mask)[0]))
    assert len(lat.points_in) == int(fx["n_inside"])


def test_clip_jobs_order():
    from oakink2_tamf_amd.metrics.siv import clip_jobs

    j = clip_jobs(45, [10, None, 7])
    assert j["frames"].tolist() == list(range(0, 45, 20)) == [0, 20, 40]
    assert j["frame_slot"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]
    assert j["hand"].tolist() == [0, 0, 1, 1] * 3 and j["obj"].tolist() == [0, 2] * 6  # ground truth first; the object without lattice is left out
    assert j["mesh_id"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5] and j["mesh_id"].dtype == np.int32
    assert j["pt_off"].tolist() == [0, 10] * 6 and j["pt_len"].tolist() == [10, 7] * 6
    assert clip_jobs(20, [3])["frames"].tolist() == [0] and clip_jobs(21, [3])["frames"].tolist() == [0, 20]
    assert clip_jobs(0, [3])["mesh_id"].shape == (0,) and clip_jobs(45, [None])["mesh_id"].shape == (0,)


def test_tslrot6d_to_transf_is_the_float32_restatement():
    from oakink2_tamf_amd.metrics.siv import tslrot6d_to_transf

    fx = load_golden("siv_clip_two_objects.npz")
    got = tslrot6d_to_transf(fx["obj_traj"][:, : int(fx["avai_len"])])
    assert got.dtype == np.float32 and np.array_equal(got, fx["transf"])


def test_eval_header_declares_exactly_the_export_list():
    from oakink2_tamf_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "tamf_eval.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(tamf_[a-z0-9_]+)\s*\(", hdr)) == set(_lib.EVAL_EXPORTS) and len(_lib.EVAL_EXPORTS) == 4
    assert len(_lib.EXPORTS) == 27 and not set(_lib.EVAL_EXPORTS) & set(_lib.EXPORTS + _lib.HOOK_EXPORTS)
    # the sampler libraries neither compile nor stamp the score kernels; the score library has its own sources and stamp
    sampler, ev = _lib.SAMPLER.sources, _lib.EVAL.sources
    assert not {"tamf_eval.hip", "tamf_voxel.h"} & set(sampler) and "tamf_voxel.h" in ev and "tamf_geom.h" in sampler
    assert "tamf_mesh.h" in ev and "tamf_mesh.h" in sampler and "tamf_geom.h" not in ev  # the include closure
    assert _lib.EVAL.stamp_path != _lib.SAMPLER.stamp_path and _lib.EVAL.digest() != _lib.SAMPLER.digest()
    lib = _lib.load_eval()
    for sym in _lib.EVAL_EXPORTS:
        getattr(lib, sym)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.EVAL_LIB_PATH], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    assert {l.split()[-1] for l in nm.stdout.splitlines() if " T " in l and l.split()[-1].startswith("tamf_")} == set(_lib.EVAL_EXPORTS)


# ---- launcher ----------------------------------------------------------------------------------------------------------------
def _tree(root):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_score_cpu as S

    return S._synthetic_tree(root)


def _launch(argv, cwd):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")]))
    return subprocess.run([sys.executable, "-m", "oakink2_tamf_amd.launch.compute_score_siv"] + argv, cwd=cwd, env=env, capture_output=True,
                          text=True, timeout=300)


def test_launcher_arguments():
    from oakink2_tamf_amd.launch import compute_score_siv as L

    cfg = L.parse_args(["--data.process_range", "a:b", "--data.cache_dict_filepath", "c.pkl", "--debug.sample_refine_filepath", "s",
                        "--mano.factory", "fake_mano:make", "--data.obj_model_loader", "oracle.fixtures:synthetic_object_mesh",
                        "--data.obj_sdf_prefix", "sdf", "--save_dir", "out", "--device", "cuda:1"])
    assert cfg["data"]["process_range"] == ["a", "b"] and cfg["data"]["obj_model_loader"] == "oracle.fixtures:synthetic_object_mesh"
    assert cfg["data"]["obj_sdf_prefix"] == os.path.abspath("sdf") and cfg["runtime"]["save_dir"] == "out"
    assert cfg["mano"]["factory"] == "fake_mano:make" and cfg["runtime"]["device"] == "cuda:1"
    d = L.parse_args([])
    assert d["data"]["obj_model_loader"] is None and d["data"]["obj_sdf_prefix"] is None
    assert d["debug"]["sample_refine_filepath"].endswith(os.path.join("sample_refine", "main", "sample", "test", "arch_mdm_l__0399"))
    v, f = L.resolve_loader("oracle.fixtures:synthetic_object_mesh")("C10001")
    assert v.shape[1] == 3 and f.shape[1] == 3 and L.resolve_loader(None) is None
    with pytest.raises(SystemExit):
        L.resolve_loader("no_colon")


def test_launcher_dry_run_and_missing_inputs(tmp_path):
    paths, cache, tree = _tree(str(tmp_path))
    data = ["--data.cache_dict_filepath", paths["cache"], "--data.obj_embedding_prefix", paths["emb"], "--data.obj_pointcloud_prefix",
            paths["pc"], "--debug.sample_refine_filepath", tree]
    r = _launch(data + ["--dry_run", "--data.obj_model_loader", "oracle.fixtures:synthetic_object_mesh"], str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    infos = cache["interaction_segment_info_list"]
    assert out["n_clips"] == 3 and [tuple(p["info"]) for p in out["pairs"]] == [tuple(infos[i]) for i in (0, 1, 2)]
    assert out["obj_model_loader"] == "oracle.fixtures:synthetic_object_mesh"
    r = _launch(data, str(tmp_path))
    assert r.returncode != 0 and "the refine stage needs MANO: pass --mano.factory module:function" in r.stderr
    r = _launch(data + ["--no_such_flag", "1", "--dry_run"], str(tmp_path))
    assert r.returncode == 2


def test_load_pairs_default_keeps_items_without_meshes(tmp_path):
    from oakink2_tamf_amd.launch import _score_common as C
    from oakink2_tamf_amd.launch import compute_score_siv as L
    from oracle.fixtures import synthetic_object_mesh

    paths, _, tree = _tree(str(tmp_path))
    cfg = L.parse_args(["--data.cache_dict_filepath", paths["cache"], "--data.obj_embedding_prefix", paths["emb"],
                        "--data.obj_pointcloud_prefix", paths["pc"], "--debug.sample_refine_filepath", tree])
    assert all("obj_verts" not in it for it, _ in C.load_pairs(cfg))
    with_mesh = C.load_pairs(cfg, obj_model_loader=synthetic_object_mesh)
    assert len(with_mesh) == 3 and all(len(it["obj_verts"]) == len(it["obj_list"]) for it, _ in with_mesh)


def test_shell_entry_point():
    path = os.path.join(ROOT, "script", "compute_score_siv.sh")
    assert os.access(path, os.X_OK)
    r = subprocess.run(["bash", path, "-n", "val", "arch_mdm_l__0399", "--mano.factory", "my.mano:make"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "oakink2_tamf_amd.launch.compute_score_siv" in r.stdout and "common/sample_refine/main/sample/val/arch_mdm_l__0399" in r.stdout
    assert subprocess.run(["bash", path, "val"], capture_output=True, text=True, timeout=60).returncode == 2
