"""CPU checks of the SegmentEncoder training step's test infrastructure and Python side: the float64 restatement against the
reference's own module and loss (tests/golden/enctrain_*.npz, captured by tools/capture_enctrain_golden.py), the label check, the
refusals of the C entry points that come before any device call, and the single place of every state-dict key in the library's source."""
import ctypes
import glob
import os
import re

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


TAMF_ERR_INVALID = -1
ARCH_FIELDS = ("input_dim", "obj_input_dim", "hand_shape_dim", "obj_embed_dim", "latent_dim", "ff_size", "num_layers", "num_heads")
HEADS_MSG = "the encoder training step supports latent_dim 64 with 4 heads, got latent_dim %d with %d heads"
FRAMES_MSG = "max_frames must be in [1, 508] (one head's keys and values in 64 KiB of LDS), got %d"


def test_create_and_mask_refusals_through_ctypes():
    """status and last_error text of every refusal of tamf_enctrain_create and tamf_enctrain_dropout_mask that returns before the
    first device call; *out, a sentinel before the call, is NULL after every refused create that was given both pointers"""
    from encoder_restatement import ARCH_ENCODER
    from oakink2_tamf_amd.hip_backend import _Arch
    from oakink2_tamf_amd.model import segment_encoder_train as ST

    lib = ST.lib()

    def create(arch=None, max_batch=4, max_frames=28, null=None):
        a = dict(ARCH_ENCODER, **(arch or {}))
        st = _Arch(*[int(a[k]) for k in ARCH_FIELDS], 0, 0, 2)
        out = ctypes.c_void_p(None if null == "arch" else 0x5A5A5A5A)  # (the null check comes before *out is written)
        rc = lib.tamf_enctrain_create(None if null == "arch" else ctypes.byref(st), max_batch, max_frames, 0, None if null == "out" else ctypes.byref(out))
        return rc, lib.tamf_enctrain_last_error().decode(), out.value

    for kw, text in ((dict(null="arch"), "null argument"), (dict(null="out"), "null argument"),
                     (dict(arch=dict(latent_dim=128)), HEADS_MSG % (128, 4)), (dict(arch=dict(num_heads=8)), HEADS_MSG % (64, 8)),
                     (dict(arch=dict(ff_size=24)), "ff_size must be a multiple of 16 in [16, 512], got 24"),
                     (dict(arch=dict(ff_size=528)), "ff_size must be a multiple of 16 in [16, 512], got 528"),
                     (dict(arch=dict(num_layers=0)), "num_layers must be in [1, 64], got 0"),
                     (dict(arch=dict(num_layers=65)), "num_layers must be in [1, 64], got 65"),
                     (dict(max_frames=0), FRAMES_MSG % 0), (dict(max_frames=509), FRAMES_MSG % 509),
                     (dict(max_batch=0), "max_batch must be in [1, 65535], got 0"),
                     (dict(max_batch=65536), "max_batch must be in [1, 65535], got 65536")):
        rc, msg, out = create(**kw)
        assert (rc, msg) == (TAMF_ERR_INVALID, text), (kw, rc, msg)
        if kw.get("null") != "out":
            assert out is None, (kw, out)  # *out == NULL

    buf = (ctypes.c_uint8 * 64)()  # never written: the arguments are checked first
    good = dict(site=0, rows=4, cols=4, p=0.5, out=ctypes.addressof(buf))
    for kw, text in ((dict(out=None), "null argument"), (dict(rows=0), "rows * cols must be in [1, 2^32)"), (dict(site=-1), "site must be >= 0"),
                     (dict(p=1.0), "p must be in [0, 1)"), (dict(p=float("nan")), "p must be in [0, 1)")):
        a = dict(good, **kw)
        rc = lib.tamf_enctrain_dropout_mask(3, 1, 2, a["site"], a["rows"], a["cols"], a["p"], a["out"], None)
        assert (rc, lib.tamf_enctrain_last_error().decode()) == (TAMF_ERR_INVALID, text), (kw, rc)
    assert not any(buf)


def test_each_key_is_written_once():
    """every key stem of the encoder's state dict - outside the layers, and of one layer - occurs exactly once in the text of
    csrc/tamf_enctrain.hip together with csrc/tamf_train_host.h (the layers' declarations): where the tensor is declared"""
    from encoder_restatement import ARCH_ENCODER, seeded_state_dict

    def stem(k):
        return re.sub(r"\.(weight|bias)$", "", k)

    layer = "seqTransEncoder.layers.0."
    keys = list(seeded_state_dict(dict(ARCH_ENCODER), 0))
    outside = sorted({stem(k) for k in keys if not k.startswith("seqTransEncoder.")})
    per_layer = sorted({stem(k[len(layer):]) for k in keys if k.startswith(layer)})
    assert len(outside) == 13 and len(per_layer) == 7, (outside, per_layer)  # (norm1 and norm2 are two of the seven)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = ""
    for name in ("tamf_enctrain.hip", "tamf_train_host.h"):
        with open(os.path.join(root, "oakink2-tamf_amd", "csrc", name)) as f:
            text += f.read()
    for s in outside + per_layer:  # (as a whole word: input_process.poseEmbedding is also the tail of obj_input_process.poseEmbedding)
        n = len(re.findall(r"(?<![A-Za-z0-9_.])" + re.escape(s) + r"(?![A-Za-z0-9_])", text))
        assert n == 1, (s, n)


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
