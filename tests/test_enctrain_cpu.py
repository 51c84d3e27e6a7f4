"""CPU checks of the SegmentEncoder training step's test infrastructure and Python side: the float64 restatement against the
reference's own module and loss (tests/golden/enctrain_*.npz, captured by tools/capture_enctrain_golden.py), the label check."""
import glob
import os

import numpy as np
import pytest

from encoder_train_restatement import load_train_case, loss_and_grads

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "enctrain_*.npz")) if "perturb" not in p)


def test_fixtures_present():
    assert len(CASES) >= 5, CASES


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference(name):
    """loss to 1e-9 relative; every gradient to 1e-9 of its tensor's largest entry, beyond the fixture's own float32 storage
    rounding (2^-24 relative per element, an exact bound); NaN entries (the non-finite case) in the same places"""
    c = load_train_case(os.path.join(GOLDEN, name))
    loss, _, grads = loss_and_grads(c["sd"], c["arch"], c["inputs"], c["labels"], c["obj_num"])
    assert abs(loss - c["loss"]) <= 1e-9 * abs(c["loss"]), (loss, c["loss"])
    assert set(grads) == set(c["grads"])
    for k, ref in c["grads"].items():
        ref = ref.astype(np.float64)
        nan = np.isnan(ref)  # (non-finite inputs: torch's weight gradients behind the nan_to_num mask are 0 * NaN)
        assert (np.isnan(grads[k]) == nan).all(), k
        if nan.all():
            continue
        err = np.abs(grads[k] - ref) - 2.0 ** -24 * np.abs(ref)
        assert np.nanmax(err) <= 1e-9 * np.nanmax(np.abs(ref)), (k, np.nanmax(err), np.nanmax(np.abs(ref)))
    assert 0 < c["tol_rel"] < 1e-4 and 0 <= c["tol_rel_loss"] < 1e-5


def test_label_range():
    from oakink2_tamf_amd.model.segment_encoder_train import check_labels

    assert check_labels([0, 98], 99).dtype == np.int64
    for bad in ([99], [0, -1], [[0]], [0.5]):
        with pytest.raises(ValueError):
            check_labels(np.asarray(bad), 99)


def test_gaussian_perturb_adaptor_equals_reference():
    """the arrays the reference's class gave under np.random.seed; unit rot6d halves on the valid frames; padded frames untouched"""
    from oakink2_tamf_amd.dataset.pose_repr_sample import GuassianPerturbSampleAdaptor

    z = np.load(os.path.join(GOLDEN, "enctrain_perturb.npz"))
    base = [{"pose_repr": z[f"pose_repr_{i}"].copy(), "len": int(z[f"len_{i}"])} for i in range(3)]
    ad = GuassianPerturbSampleAdaptor(base, tuple(z["range"]))
    assert len(ad) == 3
    np.random.seed(int(z["seed"]))
    for i in range(3):
        item = ad[i]
        n = base[i]["len"]
        got = item["sample_pose_repr"]
        assert item["sample_info"] == (i, float(z[f"sigma_{i}"]))
        assert got.dtype == z[f"sample_pose_repr_{i}"].dtype and np.array_equal(got, z[f"sample_pose_repr_{i}"])
        assert np.abs(np.linalg.norm(got[:n, 3:99].reshape(n, 32, 3), axis=-1) - 1).max() < 1e-5
        assert np.array_equal(got[n:], z[f"pose_repr_{i}"][n:]) and np.array_equal(item["pose_repr"], z[f"pose_repr_{i}"])


def test_action_list_equals_reference():
    from oakink2_tamf_amd.dataset.action_adapter import ACTION_LIST, ActionRecognitionAdapter

    with open(os.path.join(GOLDEN, "enctrain_action_list.txt")) as f:
        assert [ln.strip() for ln in f if ln.strip()] == list(ACTION_LIST)
    assert len(ACTION_LIST) == 69 and len(set(ACTION_LIST)) == 69
    ad = ActionRecognitionAdapter([{"info": ("seq", "pour:whatever")}, {"info": ("seq", "close_book")}])
    a, b = ad[0], ad[1]
    assert (a["action_label"], a["action_label_id"]) == ("pour", 2) and a["action_onehot"].sum() == 1 and a["action_onehot"][2] == 1
    assert b["action_label_id"] == 68 and len(ad) == 2
    with pytest.raises(ValueError):
        ActionRecognitionAdapter([{"info": ("seq", "juggle:x")}])[0]


def test_launcher_dry_run_lists_datasets_and_schedule(tmp_path):
    import json
    import subprocess

    from enctrain_fixture import launcher_cmd, launcher_env, write_training_tree

    paths, n = write_training_tree(str(tmp_path), n_segments=6)
    cmd = launcher_cmd(paths, "--train.batch_size", "4", "--train.num_epoch", "50", "--train.scheduler_milestone", "10,20,30",
                        "--train.scheduler_gamma", "0.5", "--train.record_freq", "20", "--dry_run")
    r = subprocess.run(cmd, capture_output=True, text=True, env=launcher_env(), cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert (info["train_identity"], info["train_generated"], info["train_gaussian_perturb"], info["train_total"]) == (n, n, n, 3 * n)
    assert info["val"] == n and info["test"] is None
    assert info["steps_per_epoch"] == (3 * n) // 4 and info["scheduler_milestone"] == [10, 20, 30]
    assert info["lr_first"] == 1e-4 and abs(info["lr_last"] - 1e-4 / 8) < 1e-12
    assert info["record_epochs"] == [0, 19, 39, 49]
    assert info["model"]["latent_dim"] == 64 and info["model"]["dropout"] == 0.1
    assert not os.path.exists(os.path.join(str(tmp_path), "common", "train_encoder"))


def test_train_encoder_sh_prints_its_command():
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["bash", os.path.join(root, "script", "train_encoder.sh"), "-n", "--runtime.seed", "3"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    for word in ("oakink2_tamf_amd.launch.train_encoder", "arch_encoder.yml", "--train.num_epoch 400", "--train.scheduler_milestone 80\\,160\\,240\\,320",
                 "--val.val_freq 20", "--test.test_freq 20", "--commit", "--runtime.seed 3"):
        assert word in r.stdout or word.replace("\\", "") in r.stdout, (word, r.stdout)
