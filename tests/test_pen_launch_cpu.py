"""CPU: `--train.loss.coef_pen_loss` / `--data.obj_sdf_prefix` on launch/train.py and launch/train_refine.py - the dry run's plan, the
refusal without the prefix, the defaults, and that with the coefficient at 0 nothing of the term is set up: no lattice set, no
`sdf_grid_id` in a batch.  The synthetic tree is tests/train_launch_fixture.py's; the pickles hold analytic sphere lattices in the layout
script/process_object_sdf.sh writes (the GPU half, tests/test_pen_launch_gpu.py, makes them with meshdist.process_sdf)."""
import json
import os
import pickle
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import sdfgrid_cases as C  # noqa: E402
import train_launch_fixture as F  # noqa: E402


def object_ids(paths):
    from oakink2_tamf_amd.dataset.interaction_segment import load_cache_dict

    return sorted(load_cache_dict(paths["cache"])["interaction_object_list"])


def write_sphere_pickles(root, ids):
    prefix = os.path.join(root, "sdf")
    os.makedirs(prefix, exist_ok=True)
    for k, oid in enumerate(ids):
        with open(os.path.join(prefix, f"{oid}.pkl"), "wb") as f:
            pickle.dump(C.fields_from(C.sphere_fn(0.05 + 0.01 * k), [0, 0, 0], [0.2, 0.2, 0.2], 8), f, protocol=4)
    return prefix


@pytest.mark.parametrize("prog", ["train", "train_refine"])
def test_dry_run_lists_the_objects_without_a_file(prog, tmp_path):
    paths = F.write_tree(str(tmp_path), mano=False)
    ids = object_ids(paths)
    assert len(ids) >= 2
    prefix = write_sphere_pickles(str(tmp_path), ids[1:])  # the first object has no file
    cmd = F.launcher_cmd(prog, paths, "--train.loss.coef_pen_loss", "0.5", "--data.obj_sdf_prefix", prefix, "--dry_run")
    r = subprocess.run(cmd, capture_output=True, text=True, env=F.launcher_env(), cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["n_objects_without_sdf"] == 1 and info["loss"]["coef_pen_loss"] == 0.5
    assert not os.path.exists(os.path.join(str(tmp_path), "common", prog))  # nothing is written
    # without the new flags the plan is what it was: no count, no coefficient
    r = subprocess.run(F.launcher_cmd(prog, paths, "--dry_run"), capture_output=True, text=True, env=F.launcher_env(), cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert "n_objects_without_sdf" not in info and "coef_pen_loss" not in info["loss"]


@pytest.mark.parametrize("prog", ["train", "train_refine"])
def test_a_positive_coefficient_without_the_prefix_is_refused(prog, tmp_path):
    import importlib

    L = importlib.import_module(f"oakink2_tamf_amd.launch.{prog}")
    paths = F.write_tree(str(tmp_path), mano=False)
    argv = F.launcher_cmd(prog, paths, "--train.loss.coef_pen_loss", "1.0", "--dry_run")[3:]
    with pytest.raises(SystemExit, match="script/process_object_sdf.sh"):
        L.main(argv)
    with pytest.raises(SystemExit, match="no directory"):
        L.main(argv + ["--data.obj_sdf_prefix", str(tmp_path / "absent")])
    os.makedirs(tmp_path / "empty")
    with pytest.raises(SystemExit, match="holds no"):
        L.main(argv + ["--data.obj_sdf_prefix", str(tmp_path / "empty")])


@pytest.mark.parametrize("prog", ["train", "train_refine"])
def test_defaults_leave_the_term_off_and_nothing_of_it_is_set_up(prog, tmp_path):
    import importlib

    import torch

    from oakink2_tamf_amd.launch import _train_common as TC

    L = importlib.import_module(f"oakink2_tamf_amd.launch.{prog}")
    paths = F.write_tree(str(tmp_path), mano=False)
    argv = F.launcher_cmd(prog, paths)[3:]
    cfg = L.parse_args(argv)
    assert float(cfg["train"]["loss"].get("coef_pen_loss", 0.0)) == 0.0 and cfg["data"]["obj_sdf_prefix"] is None and not TC.pen_on(cfg)
    assert "coef_pen_loss" not in TC.positive_coefs(cfg)
    ds, extra = L.datasets(cfg)
    assert ds.sdf_grids is None and "n_objects_without_sdf" not in extra  # no lattice set is built
    items = [ds[0], ds[1]]
    batch = TC.collate(items, "cpu", L.FIELDS, True)
    assert "sdf_grid_id" not in batch  # and none is collated

    # on: the set is read once from the distinct objects of the cache, and a batch carries its table
    ids = object_ids(paths)
    prefix = write_sphere_pickles(str(tmp_path), ids[1:])
    cfg = L.parse_args(argv + ["--train.loss.coef_pen_loss", "2", "--data.obj_sdf_prefix", prefix])
    assert cfg["train"]["loss"]["coef_pen_loss"] == 2.0 and cfg["data"]["obj_sdf_prefix"] == prefix and TC.pen_on(cfg)
    ds, extra = L.datasets(cfg)
    assert extra["n_objects_without_sdf"] == 1 and ds.sdf_grids.G == len(ids) - 1 and ds.sdf_grids.device is None  # (read, not uploaded)
    assert ds.sdf_grids.index_of == {oid: k for k, oid in enumerate(ids[1:])}
    batch = TC.collate(items, "cpu", L.FIELDS, True, ds.sdf_grids.index_of)
    table = batch["sdf_grid_id"]
    assert table.dtype == torch.int32 and tuple(table.shape) == (2, max(batch["obj_num"]))
    for b, it in enumerate(items):
        want = [ds.sdf_grids.index_of.get(o, -1) for o in it["obj_list"]]
        assert table[b].tolist() == want + [-1] * (table.shape[1] - len(want))
