"""CPU: the CR / PSKL-J evaluation away from the GPU - fixtures against the float64 restatement, pskl_terms, the C header and export
list, the launchers' --dry_run and MANO error, and the two shell entry points.

Tolerances.  The fixtures (tools/capture_score_golden.py) hold what the reference's own lines computed with numpy's float32 FFT, so
they sit about 2e-7 from exact arithmetic (measured on these fixtures: spectra 1.2e-7 .. 2.0e-7 of the feature's largest bin, scores
up to 4.2e-7 relative).  GAP_BOUND = 1e-5 is only a sanity bound on the capture, as the issue sets it.  pskl_1 / pskl_2 are float32 in
the fixture: pskl_terms (float64) on the fixture's own float32 spectra is compared after a cast to float32, within 4 ulp of float32."""
import json
import os
import pickle
import shlex
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import score_restatement as R  # noqa: E402

GAP_BOUND = 1e-5
CASES = [("psklj_t160.npz", ""), ("psklj_t7.npz", ""), ("psklj_degenerate.npz", "const/"), ("psklj_degenerate.npz", "same/")]
IDS = ["t160", "t7", "degenerate-const", "degenerate-same"]


def load_case(name, prefix):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix) and k != "numpy_version"}


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def fixture_gaps(fx):
    """max |reference - float64 restatement|: summed spectra relative to each feature's largest bin, scores relative"""
    ds, ms = R.spectrum_sum(fx["dataset_joints"], fx["lens"]), R.spectrum_sum(fx["model_joints"], fx["lens"])
    g_spec = max(R.rel_to_feature_max(fx["dataset_psd"].astype(np.float64).sum(axis=0), ds),
                 R.rel_to_feature_max(fx["model_psd"].astype(np.float64).sum(axis=0), ms))
    p = R.pskl(ds, ms)
    g_score = max(rel(p[0], float(fx["pskl_1"])), rel(p[1], float(fx["pskl_2"])))
    return g_spec, g_score


@pytest.mark.parametrize("name,prefix", CASES, ids=IDS)
def test_restatement_matches_reference_fixture(name, prefix):
    fx = load_case(name, prefix)
    T = fx["dataset_joints"].shape[1]
    assert fx["dataset_psd"].shape == (fx["dataset_joints"].shape[0], T - 2, 21, 3)
    g_spec, g_score = fixture_gaps(fx)
    print(f"{name} {prefix}: gap spectra {g_spec:.3e} scores {g_score:.3e}")
    assert g_spec < GAP_BOUND and g_score < GAP_BOUND
    # per clip too (what the kernel's psd_clip output is held against)
    for key, joints in (("dataset_psd", "dataset_joints"), ("model_psd", "model_joints")):
        mine = R.clip_spectra(fx[joints], fx["lens"])
        for n in range(mine.shape[0]):
            assert R.rel_to_feature_max(fx[key][n].astype(np.float64), mine[n]) < GAP_BOUND


@pytest.mark.parametrize("name,prefix", CASES, ids=IDS)
def test_pskl_terms_reproduces_reference_scores(name, prefix):
    from oakink2_tamf_amd.metrics.psklj import pskl_terms

    fx = load_case(name, prefix)
    t = pskl_terms(np.sum(fx["dataset_psd"], axis=0), np.sum(fx["model_psd"], axis=0))
    assert t["n_freq"] == fx["dataset_psd"].shape[1] and t["n_feat"] == 21
    for got, want in ((t["pskl_gt_model"], fx["pskl_1"]), (t["pskl_model_gt"], fx["pskl_2"])):
        want = np.float32(want)
        assert want.dtype == np.float32
        assert abs(float(np.float32(got)) - float(want)) <= 4 * float(np.spacing(np.abs(want))), (got, want)  # 4 ulp of float32
    # the restatement agrees with the product's host arithmetic exactly (same operations, same order)
    assert (t["pskl_gt_model"], t["pskl_model_gt"]) == R.pskl(np.sum(fx["dataset_psd"], axis=0), np.sum(fx["model_psd"], axis=0))


def test_pskl_terms_identical_sets_and_constant_set():
    from oakink2_tamf_amd.metrics.psklj import EPS, pskl_terms

    fx = load_case("psklj_degenerate.npz", "same/")
    s = R.spectrum_sum(fx["dataset_joints"], fx["lens"])
    t = pskl_terms(s, s.copy())
    assert t["pskl_gt_model"] == 0.0 and t["pskl_model_gt"] == 0.0
    fx = load_case("psklj_degenerate.npz", "const/")
    d, m = R.spectrum_sum(fx["dataset_joints"], fx["lens"]), R.spectrum_sum(fx["model_joints"], fx["lens"])
    assert not d.any() and m.any()  # a set constant in time has no acceleration: the 1e-8 alone decides
    L = d.shape[0]
    uniform = (d + EPS) / np.sum(d + EPS, axis=0, keepdims=True)
    np.testing.assert_array_equal(uniform, np.full_like(uniform, uniform.flat[0]))
    assert abs(uniform.flat[0] - 1.0 / L) < 1e-15
    mn = (m + EPS) / np.sum(m + EPS, axis=0, keepdims=True)
    want = float(np.sum(np.log(1.0 / L / mn)) / L / 21)  # KL(uniform || model), per joint
    assert abs(pskl_terms(d, m)["pskl_gt_model"] - want) < 1e-12 * abs(want)
    with pytest.raises(ValueError):
        pskl_terms(d, m[:-1])


def test_direct_dft_restatement_sits_on_the_fft():
    """the yardstick of the GPU bound (64 x this gap, floor 1e-13): a correct direct float64 DFT vs np.fft.fft on the fixtures"""
    for (name, prefix), tag in zip(CASES, IDS):
        fx = load_case(name, prefix)
        g = R.rel_to_feature_max(R.direct_dft_spectra(fx["model_joints"], fx["lens"]).sum(axis=0), R.spectrum_sum(fx["model_joints"], fx["lens"]))
        print(f"{tag}: direct DFT vs FFT {g:.3e}")
        assert g < 1e-13


def test_header_and_export_list_name_the_entry_point():
    from oakink2_tamf_amd import _lib

    with open(os.path.join(ROOT, "include", "tamf_hip.h")) as f:
        assert "int tamf_power_spectrum_sum(" in f.read()
    assert "tamf_power_spectrum_sum" in _lib.EXPORTS and len(_lib.EXPORTS) == 27
    assert "tamf_spectrum.h" in _lib.SAMPLER.sources


def test_power_spectrum_sum_rejects_unequal_clips():
    import torch

    from oakink2_tamf_amd.metrics.psklj import power_spectrum_sum

    with pytest.raises(ValueError, match="unequal"):
        power_spectrum_sum([torch.zeros(8, 21, 3), torch.zeros(9, 21, 3)])


# ---- launchers -------------------------------------------------------------------------------------------------------------
def _synthetic_tree(root):
    """oracle.fixtures' synthetic segment cache (5 segments; 2 and 3 share one `info`) and a sample_refine tree holding save dicts for
    segments 0, 1 and 2 - segment 4 has none"""
    from oakink2_tamf_amd.launch import formats
    from oracle import fixtures

    paths, cache = fixtures.write_synthetic_dataset(root)
    infos = cache["interaction_segment_info_list"]
    assert tuple(infos[2]) == tuple(infos[3]) and len({tuple(i) for i in infos}) == 4
    tree = os.path.join(root, "srf")
    rng = np.random.default_rng(5)
    for i in (0, 1, 2):
        T = 160
        d = formats.build_refine_save_dict(infos[i], infos[i][2], rng.normal(size=(T, 21, 3)).astype(np.float32),
                                           rng.normal(size=(T, 778, 3)).astype(np.float32), None,
                                           sorted(cache["interaction_segment_obj_traj_list"][i]), cache["interaction_segment_len_list"][i],
                                           cache["interaction_segment_frame_id_list"][i], np.zeros((T, 99), np.float32))
        path = formats.refine_sample_path_in(tree, infos[i])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            pickle.dump(d, f)
    return paths, cache, tree


def _launch(module, argv, cwd):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")]))
    return subprocess.run([sys.executable, "-m", "oakink2_tamf_amd.launch." + module] + argv, cwd=cwd, env=env, capture_output=True,
                          text=True, timeout=300)


def _data_args(paths, tree):
    return ["--data.cache_dict_filepath", paths["cache"], "--data.obj_embedding_prefix", paths["emb"], "--data.obj_pointcloud_prefix",
            paths["pc"], "--debug.sample_refine_filepath", tree]


@pytest.mark.parametrize("module", ["compute_score_cr", "compute_score_psklj"])
def test_dry_run_lists_the_pairs(tmp_path, module):
    paths, cache, tree = _synthetic_tree(str(tmp_path))
    r = _launch(module, _data_args(paths, tree) + ["--dry_run"], str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    infos = cache["interaction_segment_info_list"]
    assert out["n_clips"] == 3 and [tuple(p["info"]) for p in out["pairs"]] == [tuple(infos[i]) for i in (0, 1, 2)]
    assert [p["len"] for p in out["pairs"]] == [cache["interaction_segment_len_list"][i] for i in (0, 1, 2)]
    assert all(os.path.isfile(p["save_dict"]) for p in out["pairs"])


@pytest.mark.parametrize("module", ["compute_score_cr", "compute_score_psklj"])
def test_missing_mano_factory_is_the_sample_refine_message(tmp_path, module):
    paths, _, tree = _synthetic_tree(str(tmp_path))
    r = _launch(module, _data_args(paths, tree), str(tmp_path))
    assert r.returncode != 0
    assert "the refine stage needs MANO: pass --mano.factory module:function" in r.stderr
    r = _launch(module, _data_args(paths, tree) + ["--no_such_flag", "1", "--dry_run"], str(tmp_path))
    assert r.returncode == 2  # unknown flags are an error


def test_launchers_mirror_the_reference_argument_names():
    from oakink2_tamf_amd.launch import compute_score_cr, compute_score_psklj

    for mod in (compute_score_cr, compute_score_psklj):
        cfg = mod.parse_args(["--data.data_prefix", "d", "--data.process_range", "a:b", "--data.obj_embedding_prefix", "e",
                              "--data.obj_pointcloud_prefix", "p", "--data.cache_dict_filepath", "c.pkl", "--debug.sample_refine_filepath",
                              "s", "--mano.mano_path", "m", "--mano.factory", "fake_mano:make", "--batch_size", "7", "--device", "cuda:1"])
        assert cfg["data"]["process_range"] == ["a", "b"] and cfg["data"]["cache_dict_filepath"] == os.path.abspath("c.pkl")
        assert cfg["mano"]["factory"] == "fake_mano:make" and cfg["mano"]["mano_path"] == os.path.abspath("m")
        assert cfg["runtime"]["batch_size"] == 7 and cfg["runtime"]["device"] == "cuda:1"
        d = mod.parse_args([])
        assert d["data"]["cache_dict_filepath"].endswith(os.path.join("common", "save_cache_dict", "main", "cache", "test.pkl"))
        assert d["debug"]["sample_refine_filepath"].endswith(os.path.join("sample_refine", "main", "sample", "test", "arch_mdm_l__0399"))
        with pytest.raises(SystemExit):
            mod.parse_args(["--debug.cache_dict_filepath", "c.pkl"])  # the FID script's spelling, not these scripts'
    assert compute_score_cr.parse_args(["--save_dir", "x"])["runtime"]["save_dir"] == "x"


@pytest.mark.parametrize("script,module", [("compute_score_cr.sh", "compute_score_cr"), ("compute_score_psklj.sh", "compute_score_psklj")])
def test_shell_entry_points(script, module):
    import importlib

    path = os.path.join(ROOT, "script", script)
    assert os.access(path, os.X_OK)
    r = subprocess.run(["bash", path, "-n", "val", "arch_mdm_l__0399", "--mano.factory", "my.mano:make", "--batch_size", "32"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "split:" in r.stdout and "model_name:" in r.stdout
    toks = shlex.split([l for l in r.stdout.splitlines() if l.startswith("python -m ")][-1])
    assert toks[:3] == ["python", "-m", "oakink2_tamf_amd.launch." + module]
    assert toks[3:] == ["--data.process_range", "?(file:./asset/split/val.txt)", "--data.cache_dict_filepath",
                        "common/save_cache_dict/main/cache/val.pkl", "--debug.sample_refine_filepath",
                        "common/sample_refine/main/sample/val/arch_mdm_l__0399", "--mano.factory", "my.mano:make", "--batch_size", "32"]
    mod = importlib.import_module("oakink2_tamf_amd.launch." + module)
    ap_args = [t for t in toks[3:]]
    ap_args[1] = "scene_a:scene_b"  # (the ?(file:...) macro needs the split file; the parser takes the rest as it is)
    cfg = mod.parse_args(ap_args)
    assert cfg["mano"]["factory"] == "my.mano:make" and cfg["runtime"]["batch_size"] == 32
    assert cfg["debug"]["sample_refine_filepath"].endswith("common/sample_refine/main/sample/val/arch_mdm_l__0399")
    r = subprocess.run(["bash", path, "val"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr
    r = subprocess.run(["bash", path, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "split" in r.stdout
