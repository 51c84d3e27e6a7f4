"""The optimiser step without a GPU: the float64 restatement against torch's own definition, the library's description in _lib, the
built library's exports, HipAdamW's refusals, and the train / train_refine launchers' dry runs (script -n, launcher --dry_run)."""
import json
import os
import re
import shlex
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")) if p not in sys.path]

import optim_restatement as R  # noqa: E402


# ---- the restatement is torch's definition ----------------------------------------------------------------------------------------

def _hip_defaults():
    """HipAdamW's own hyper-parameters (a CPU construction, no GPU): the restatement is compared with torch at THESE"""
    import torch

    from oakink2_tamf_amd.optim import HipAdamW

    opt = HipAdamW([torch.nn.Parameter(torch.zeros(1))], clip_max_norm=0.1)
    g = opt.param_groups[0]
    return dict(lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"]), opt.clip_max_norm


@pytest.mark.parametrize("weight_decay,clip", [(0.0, True), (0.01, True), (0.01, False)])
def test_restatement_equals_torch_float64(weight_decay, clip):
    """clip_grad_norm_ per parameter + torch.optim.AdamW in float64 against the numpy formulas at HipAdamW's defaults (and ten times
    its lr), to 1e-12 relative; clipped and unclipped steps both occur"""
    import torch

    hyper, max_norm = _hip_defaults()
    assert (hyper, max_norm) == (dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8), 0.1)
    max_norm = max_norm if clip else None
    rng = np.random.default_rng(11)
    sizes = [1, 5, 64, 1000, (33, 17)]
    ps = [rng.standard_normal(s) for s in sizes]
    steps = []
    for _ in range(12):
        steps.append([rng.standard_normal(p.shape) * 10.0 ** rng.uniform(-4, 1) / np.sqrt(p.size) for p in ps])
    norms = np.array([[R.grad_norm(g) for g in gs] for gs in steps])
    assert (norms > 0.1).any() and (norms < 0.1).any()
    for lr in (hyper["lr"], 10 * hyper["lr"]):
        kw = dict(hyper, lr=lr, weight_decay=weight_decay, max_norm=max_norm)
        ref, state = R.run(ps, steps, **kw)
        params, opt = R.torch_run(ps, steps, torch.float64, **kw)
        for p, r, (m, v, t) in zip(params, ref, state):
            st = opt.state[p]
            assert t == 12 and float(st["step"]) == 12
            assert R.rel_err(p.detach().numpy(), r) < 1e-12
            assert R.rel_err(st["exp_avg"].numpy(), m) < 1e-12
            assert R.rel_err(st["exp_avg_sq"].numpy(), v) < 1e-12


def test_restatement_nan_gradient_poisons_its_tensor_only():
    """the restatement's NaN rule is torch's (clamp keeps a NaN coefficient), at HipAdamW's defaults"""
    import torch

    hyper, max_norm = _hip_defaults()
    ps = [np.ones(4), np.ones(3)]
    gs = [[np.array([1.0, np.nan, 0.0, 2.0]), np.array([1.0, 2.0, 3.0])]]
    ref, state = R.run(ps, gs, max_norm=max_norm, **hyper)
    params, opt = R.torch_run(ps, gs, torch.float64, max_norm=max_norm, **hyper)
    assert np.isnan(ref[0]).all() and np.isnan(state[0][0]).all() and np.isnan(state[0][1]).all()
    assert np.isnan(params[0].detach().numpy()).all() and np.isnan(opt.state[params[0]]["exp_avg_sq"].numpy()).all()
    assert np.isfinite(ref[1]).all() and R.rel_err(params[1].detach().numpy(), ref[1]) < 1e-12


# ---- the library's description ----------------------------------------------------------------------------------------------------

def test_lib_description():
    from oakink2_tamf_amd import _lib

    with open(os.path.join(_lib.INCLUDE, "tamf_optim.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(tamf_optim_\w+)\s*\(", text))) == sorted(_lib.OPTIM_EXPORTS)
    lib = _lib.OPTIM
    assert _lib.OPTIMISER == (lib,)
    old = _lib.LIBRARIES + _lib.PREPROCESSING + _lib.TEXT_PREPROCESSING + _lib.TRAINING + _lib.REFINE_TRAINING + _lib.DENOISER_TRAINING
    assert lib not in old and len(old) == 9
    assert (_lib.LIBRARIES, _lib.PREPROCESSING, _lib.TEXT_PREPROCESSING) == ((_lib.SAMPLER, _lib.EVAL, _lib.MANO), (_lib.POINTENC,), (_lib.TEXTENC,))
    assert (_lib.TRAINING, _lib.REFINE_TRAINING, _lib.DENOISER_TRAINING) == ((_lib.ENCTRAIN, _lib.CONTACT), (_lib.REFINETRAIN,), (_lib.MDMTRAIN,))
    assert lib.root == "tamf_optim.hip" and lib.headers == ("tamf_optim.h", "tamf_hip.h")
    assert [o.file for o in lib.outputs] == ["libtamf_optim.so"] and lib.outputs[0].exports == _lib.OPTIM_EXPORTS
    assert _lib.OPTIM_LIB_PATH == lib.paths[0]
    assert lib.sources == ["tamf_optim.h", "tamf_optim.hip"]  # none of the sampler's or the training steps' host headers
    assert len(lib.kernels) >= 2 and not lib.counted_waits
    assert not any(set(o.exports) & set(_lib.OPTIM_EXPORTS) for l in old for o in l.outputs)
    import inspect

    assert "OPTIMISER" in inspect.getsource(_lib.build) and callable(_lib.load_optim)


def test_built_library_exports_the_headers_functions():
    """nm -D of the built library: exactly the header's functions among the tamf_* symbols"""
    import shutil

    from oakink2_tamf_amd import _lib

    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    path = _lib.OPTIM.build()
    res = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True)
    syms = sorted(ln.split()[-1] for ln in res.stdout.splitlines() if ln.split() and ln.split()[-1].startswith("tamf_"))
    assert syms == sorted(_lib.OPTIM_EXPORTS)


def test_header_chunk_is_the_kernels():
    from oakink2_tamf_amd import _lib

    with open(os.path.join(_lib.INCLUDE, "tamf_optim.h")) as f:
        pub = int(re.search(r"#define\s+TAMF_OPTIM_CHUNK\s+(\d+)", f.read()).group(1))
    with open(os.path.join(_lib.CSRC, "tamf_optim.h")) as f:
        dev = int(re.search(r"constexpr int OPT_CHUNK = (\d+);", f.read()).group(1))
    assert pub == dev


# ---- HipAdamW's refusals: raised before any GPU use -------------------------------------------------------------------------------

def test_hipadamw_refusals():
    import torch

    from oakink2_tamf_amd.optim import HipAdamW

    w = torch.nn.Parameter(torch.zeros(4, 3))
    for flag in ("amsgrad", "maximize", "capturable"):
        with pytest.raises(ValueError, match=flag):
            HipAdamW([w], **{flag: True})
    with pytest.raises(ValueError, match="float32"):
        HipAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(ValueError, match="float32"):
        HipAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))])
    with pytest.raises(ValueError, match="contiguous"):
        HipAdamW([torch.nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(ValueError, match="clip_max_norm"):
        HipAdamW([w], clip_max_norm=-1.0)
    with pytest.raises(TypeError):
        HipAdamW([w], nesterov=True)
    opt = HipAdamW([w], clip_max_norm=0.1)
    with pytest.raises(ValueError, match="contiguous"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(4, 6).t())]})


def test_hipadamw_is_torch_adamw_for_state_and_schedulers():
    """an AdamW by inheritance: the defaults, the state dict layout and MultiStepLR are torch's; flags that arrive through
    load_state_dict are refused at the step, before the device is touched"""
    import torch

    from oakink2_tamf_amd.optim import HipAdamW

    w, b = torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(3))
    opt = HipAdamW([w, b], clip_max_norm=0.1)
    assert isinstance(opt, torch.optim.AdamW) and opt.clip_max_norm == 0.1
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (1e-4, (0.9, 0.999), 1e-8, 0.0)
    ref = torch.optim.AdamW([w, b], lr=1e-4, weight_decay=0.0)
    assert set(opt.state_dict()["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.5)
    opt.step()  # no gradient anywhere: nothing to do, no state, no GPU
    sched.step()
    assert opt.param_groups[0]["lr"] == 5e-5 and len(opt.state) == 0
    sd = ref.state_dict()
    sd["param_groups"][0]["amsgrad"] = True
    opt.load_state_dict(sd)
    w.grad = torch.zeros_like(w)
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()


# ---- the launchers' dry runs ------------------------------------------------------------------------------------------------------

def _sh(script, *args):
    r = subprocess.run(["bash", os.path.join(ROOT, "script", script), *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    toks = shlex.split([l for l in r.stdout.splitlines() if l.startswith("python -m ")][-1])
    return toks[2], toks[3:]


def test_train_sh_prints_a_command_the_launcher_parses():
    from oakink2_tamf_amd.launch import train as L

    module, argv = _sh("train.sh", "-n", "--train.num_epoch", "3")
    assert module == "oakink2_tamf_amd.launch.train"
    cfg = L.parse_args(argv)
    assert cfg["ckpt"]["commit"] and cfg["ckpt"]["exp_id"].startswith("main__") and "?(ts)" not in cfg["ckpt"]["exp_id"]
    assert cfg["model"]["latent_dim"] == 512 and cfg["model"]["ff_size"] == 2048  # arch_mdm_l
    t = cfg["train"]
    assert (t["batch_size"], t["num_epoch"], t["optimizer"], t["start_epoch"]) == (64, 3, "hip", 0)
    assert t["cache_dict_filepath"].endswith("common/save_cache_dict/main/cache/train.pkl")
    assert t["loss"] == {"vpe_path": os.path.abspath("asset/grabnet/verts_per_edge.npy"), "c_weight_path": os.path.abspath("asset/grabnet/rhand_weight.npy"),
                         "coef_rec_joint_loss": 1.0, "coef_rec_vert_loss": 1.0, "coef_edge_len_loss": 0.1, "coef_dist_h_loss": 0.1, "coef_dist_o_loss": 1.0}
    assert cfg["data"]["append_reverse_segment"] and cfg["data"]["obj_embedding_prefix"] and cfg["data"]["obj_pointcloud_prefix"]
    assert cfg["data"]["text_embedding_filepath"].endswith("text_embedding.pkl")
    assert cfg["mano"]["factory"] == "oakink2_tamf_amd.mano:make_mano_differentiable" and cfg["runtime"]["device_id"] == [0]
    assert (cfg["val"]["val_freq"], cfg["test"]["test_freq"]) == (-1, -1)


def test_train_refine_sh_prints_a_command_the_launcher_parses():
    from oakink2_tamf_amd.launch import train_refine as L

    module, argv = _sh("train_refine.sh", "-n", "--train.optimizer", "torch")
    assert module == "oakink2_tamf_amd.launch.train_refine"
    cfg = L.parse_args(argv)
    t = cfg["train"]
    assert cfg["ckpt"]["commit"] and cfg["ckpt"]["exp_id"].startswith("refine__") and t["optimizer"] == "torch"
    assert cfg["model"]["latent_dim"] == 256 and t["batch_size"] == 64
    assert [os.path.basename(p) for p in t["data"]["pose_repr_sample_dir_list"]] == ["arch_mdm_l__0099"] and t["data"]["gaussian_perturb_range"] == [0.02, 0.1]
    assert {k: v for k, v in t["loss"].items() if k.startswith("coef_")} == {"coef_rec_joint_loss": 1.0, "coef_rec_vert_loss": 1.0, "coef_dist_h_loss": 0.1}
    assert (cfg["val"]["val_freq"], cfg["test"]["test_freq"]) == (20, 40)
    with pytest.raises(SystemExit):
        L.parse_args(argv + ["--train.optimizer", "sgd"])
    with pytest.raises(SystemExit):
        L.parse_args(argv + ["--train.loss.coef_dist_o_loss", "1.0"])  # (not a term of the refiner's loss)


@pytest.mark.parametrize("prog", ["train", "train_refine"])
def test_launcher_dry_run_on_a_synthetic_cache(prog, tmp_path):
    """--dry_run: sizes, steps per epoch and the schedule, without a GPU and without MANO"""
    import train_launch_fixture as F

    paths = F.write_tree(str(tmp_path), mano=False)
    cmd = F.launcher_cmd(prog, paths, "--train.num_epoch", "7", "--train.scheduler_milestone", "2,5", "--train.record_freq", "3", "--dry_run")
    if prog == "train":
        cmd.append("--data.append_reverse_segment")
    r = subprocess.run(cmd, capture_output=True, text=True, env=F.launcher_env(), cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    n = 2 * F.SEGMENTS  # G: the segments and their reversed twins; R: generated samples + Gaussian perturbation
    assert info["train_total"] == n and info["batch_size"] == F.BATCH and info["steps_per_epoch"] == n // F.BATCH and info["frames"] == F.FRAMES
    assert info["num_epoch"] == 7 and info["scheduler_milestone"] == [2, 5] and info["record_epochs"] == [0, 2, 5, 6]
    assert info["lr_first"] == 1e-4 and info["lr_last"] == 1e-4 * 0.5 * 0.5 and info["optimizer"] == "hip"
    assert info["val"] == "not run" and info["test"] == "not run" and info["model"]["latent_dim"] == 128
    if prog == "train":
        assert info["append_reverse_segment"] and info["extra_loss"] == sorted(F.COEFS["train"]) and info["prompts"] >= 1
    else:
        assert (info["train_generated"], info["train_gaussian_perturb"]) == (F.SEGMENTS, F.SEGMENTS)
    assert not os.path.exists(os.path.join(str(tmp_path), "common", prog))  # nothing is written


def test_schedule_is_a_function_of_the_epoch():
    """lr_at is MultiStepLR's lr at the start of an epoch, so a run resumed at epoch E continues the uninterrupted schedule"""
    import torch

    from oakink2_tamf_amd.launch import _train_common as C

    w = torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.AdamW([w], lr=C.BASE_LR)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2, 3, 7], gamma=0.3)
    for epoch in range(9):
        assert opt.param_groups[0]["lr"] == C.lr_at(epoch, [2, 3, 7], 0.3)
        opt.step()
        sched.step()
