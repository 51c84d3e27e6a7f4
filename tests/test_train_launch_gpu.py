"""launch/train.py and launch/train_refine.py end to end on the MI355X, as subprocesses (every launcher run is a fresh child under a
time limit; nothing in this file itself computes on the GPU): 2 epochs on the synthetic tree of tests/train_launch_fixture.py - a
tiny architecture, 16 frames, batch 2, MANO from the arrays of tests/mano_fixture.py, every loss coefficient positive.

The torch-against-hip comparison, in two parts.

One optimiser step (the parity gate).  With one batch holding the whole training set and one epoch, the `hip` and the `torch` run of
the same command take exactly one step from the same weights on the same gradient bits (the launchers are deterministic: the resume
test shows it), so their model_0000.pt differ by the optimiser alone.  Both are held, on every element, to the project's standing
gate against the float64 restatement of tests/optim_restatement.py: 4 x the error of torch's own float32 CPU AdamW step on the same
inputs, never below one float32 ulp of the tensor's largest magnitude.  The inputs: the initial weights, rebuilt here from the run's
seed (checked: no element may have moved by more than the lr, which a wrong rebuild would miss by orders of magnitude), and the
clipped gradient, read back from the torch run's exp_avg = (1 - beta1) g' after its one step.  The restatement and the yardstick
take g' as given, without clipping again; the clip itself is pinned in tests/test_optim_gpu.py.

Two epochs (a coarse check, NOT the parity gate).  After the first step the two runs' parameters differ at rounding level and the
gradients follow, so an optimiser-level gate no longer applies: elements whose true gradient is zero (the key third of every
in_proj_bias: softmax ignores a shift of the keys) carry rounding noise that AdamW normalises to O(1) updates in ANY float32 run.
On the elements whose root-mean-square gradient (sqrt of the run's exp_avg_sq) is at least 10^-3 of its tensor's largest, rounding
moves the normalised update by about 10^-3 or less, while a semantic difference between the optimisers - a missing clip, a wrong
bias correction, a stale learning rate - moves it by O(1); those elements are held to 1 % of steps x lr.  Guards against a vacuous
mask: it must keep at least a quarter of every tensor and nine tenths of all elements (the known noise, a third of the in_proj_bias
vectors, is far below a tenth).  The figures of the remaining elements are printed, not asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import optim_restatement as R  # noqa: E402
import train_launch_fixture as F  # noqa: E402

pytestmark = pytest.mark.gpu
EPOCHS = 2
LIMIT = 240  # seconds per child


def _run(prog, paths, cwd, exp_id, *extra):
    cmd = F.launcher_cmd(prog, paths, "--train.num_epoch", str(EPOCHS), "--exp_id", exp_id, "--commit", *extra)
    r = subprocess.run(cmd, capture_output=True, text=True, env=F.launcher_env(), cwd=cwd, timeout=LIMIT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return os.path.join(cwd, "common", prog, exp_id, "save"), r.stdout + r.stderr


@pytest.fixture(scope="module", params=["train", "train_refine"])
def runs(request, tmp_path_factory):
    """the uninterrupted hip run, the run resumed for the second epoch, and the torch run of the same command"""
    prog = request.param
    cwd = str(tmp_path_factory.mktemp(prog))
    paths = F.write_tree(cwd)
    full, log = _run(prog, paths, cwd, "full")
    resumed, _ = _run(prog, paths, cwd, "resumed", "--train.start_epoch", "1", "--train.reload_ckpt_model_filepath", os.path.join(full, "model_0000.pt"),
                      "--train.reload_ckpt_optimizer_filepath", os.path.join(full, "optimizer_0000.pt"))
    torch_run, _ = _run(prog, paths, cwd, "torch", "--train.optimizer", "torch")
    return {"prog": prog, "full": full, "resumed": resumed, "torch": torch_run, "log": log}


def _load(path):
    import torch

    return torch.load(path, map_location="cpu")


def test_checkpoints_are_written_and_load_into_the_inference_module(runs):
    import torch

    assert sorted(os.listdir(runs["full"])) == ["model_0000.pt", "model_0001.pt", "optimizer_0000.pt", "optimizer_0001.pt"]
    sd0, sd1 = _load(os.path.join(runs["full"], "model_0000.pt")), _load(os.path.join(runs["full"], "model_0001.pt"))
    assert set(sd0) == set(sd1) and not any(k.startswith("clip_model.") for k in sd1)
    assert all(torch.isfinite(v).all() for v in sd1.values())
    moved = [k for k in sd1 if not torch.equal(sd0[k], sd1[k])]
    assert moved and all(torch.equal(sd0[k], sd1[k]) for k in sd1 if k.endswith(".pe") or k.endswith("_embed"))  # (buffers stay)
    arch = dict(latent_dim=128, ff_size=256, num_layers=2, num_heads=2)
    if runs["prog"] == "train":
        from oakink2_tamf_amd.model.interaction_segment_mdm import InterationSegmentMDM as Module

        module = Module(**arch)
    else:
        from oakink2_tamf_amd.model.segment_refine_model import SegmentRefineModel as Module

        module = Module(None, **arch, use_pc=True)
    missing, unexpected = module.load_state_dict(sd1, strict=False)
    assert not unexpected and not [k for k in missing if not k.startswith("clip_model")]
    opt = _load(os.path.join(runs["full"], "optimizer_0001.pt"))
    n_params = len([k for k, _ in module.named_parameters() if not k.startswith("clip_model.")])
    steps = EPOCHS * (2 * F.SEGMENTS // F.BATCH if runs["prog"] == "train_refine" else F.SEGMENTS // F.BATCH)
    assert len(opt["state"]) == n_params and all(float(s["step"]) == steps for s in opt["state"].values())
    assert "val: not run" in runs["log"] and "test: not run" in runs["log"]


def test_resumed_run_repeats_the_uninterrupted_one_bit_for_bit(runs):
    import torch

    assert sorted(os.listdir(runs["resumed"])) == ["model_0001.pt", "optimizer_0001.pt"]
    a, b = _load(os.path.join(runs["full"], "model_0001.pt")), _load(os.path.join(runs["resumed"], "model_0001.pt"))
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    oa, ob = _load(os.path.join(runs["full"], "optimizer_0001.pt")), _load(os.path.join(runs["resumed"], "optimizer_0001.pt"))
    assert all(torch.equal(oa["state"][i][k], ob["state"][i][k]) for i in oa["state"] for k in ("step", "exp_avg", "exp_avg_sq"))
    assert oa["param_groups"][0]["lr"] == ob["param_groups"][0]["lr"]


def _initial_weights(prog, seed=0):
    """the weights a launcher starts from: torch.manual_seed(seed), then the module's constructor, on the CPU"""
    import torch

    arch = dict(latent_dim=128, ff_size=256, num_layers=2, num_heads=2)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        if prog == "train":
            from oakink2_tamf_amd.model.interaction_segment_mdm import InterationSegmentMDM

            module = InterationSegmentMDM(**arch)
        else:
            from oakink2_tamf_amd.model.segment_refine_model import SegmentRefineModel

            module = SegmentRefineModel(None, **arch, use_pc=True)
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


@pytest.mark.parametrize("prog", ["train", "train_refine"])
def test_one_step_of_the_torch_and_the_hip_run_inside_the_parity_gate(prog, tmp_path):
    import torch

    cwd = str(tmp_path)
    paths = F.write_tree(cwd)
    n = F.SEGMENTS if prog == "train" else 2 * F.SEGMENTS  # one batch = the whole training set: one step per epoch
    saves = {}
    for kind in ("hip", "torch"):
        cmd = F.launcher_cmd(prog, paths, "--train.num_epoch", "1", "--train.batch_size", str(n), "--train.optimizer", kind, "--exp_id", kind, "--commit")
        r = subprocess.run(cmd, capture_output=True, text=True, env=F.launcher_env(), cwd=cwd, timeout=LIMIT)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        saves[kind] = os.path.join(cwd, "common", prog, kind, "save")
    hip, ref = _load(os.path.join(saves["hip"], "model_0000.pt")), _load(os.path.join(saves["torch"], "model_0000.pt"))
    opt = _load(os.path.join(saves["torch"], "optimizer_0000.pt"))
    start = _initial_weights(prog)
    names = [k for k in ref if not (k.endswith(".pe") or k.endswith("_embed"))]  # the parameters, in named_parameters() order
    assert set(start) == set(ref) == set(hip) and len(names) == len(opt["state"])
    assert all(float(s["step"]) == 1 for s in opt["state"].values())
    lr, w1 = 1e-4, np.float64(np.float32(0.1))  # (1 - beta1 as the float32 the update multiplies by)
    for k in ref:
        if k not in names:
            assert torch.equal(start[k], ref[k]) and torch.equal(start[k], hip[k]), k
    for i, k in enumerate(names):
        p0 = start[k].numpy()
        for run in (ref, hip):  # the rebuilt weights ARE the run's: one AdamW step moves no element by more than the lr
            assert float((run[k].double() - start[k].double()).abs().max()) <= lr * (1 + 1e-3), k
        g = opt["state"][i]["exp_avg"].double().numpy() / w1  # the clipped gradient of the step
        assert g.shape == p0.shape
        r64, _ = R.run([p0], [[g]], lr=lr, max_norm=None)
        t32, _ = R.torch_run([p0], [[g.astype(np.float32)]], torch.float32, lr=lr, max_norm=None)
        bound, yard = _gate(r64[0], t32[0].detach().numpy())
        e_hip = float(np.max(np.abs(hip[k].double().numpy() - r64[0])))
        e_ref = float(np.max(np.abs(ref[k].double().numpy() - r64[0])))
        print(f"{k}: hip {e_hip:.3e} torch on the device {e_ref:.3e} against float64; torch float32 on the CPU {yard:.3e}, gate {bound:.3e}")
        assert e_hip <= bound, (k, e_hip, bound)
        assert e_ref <= bound, (k, e_ref, bound)


def _gate(ref, yard):
    """4 x the yardstick's error against `ref`, not below one float32 ulp of ref's largest magnitude; -> (gate, yardstick error)"""
    ref = np.asarray(ref, np.float64)
    e = float(np.max(np.abs(np.asarray(yard, np.float64) - ref)))
    return max(4.0 * e, float(np.spacing(np.float32(np.max(np.abs(ref)))))), e


def test_two_epochs_of_the_torch_and_the_hip_run_stay_together(runs):
    """the coarse multi-step check of the docstring: not the parity gate"""
    import torch

    hip, ref = _load(os.path.join(runs["full"], "model_0001.pt")), _load(os.path.join(runs["torch"], "model_0001.pt"))
    opt = _load(os.path.join(runs["full"], "optimizer_0001.pt"))
    names = [k for k in hip if not (k.endswith(".pe") or k.endswith("_embed"))]  # the parameters, in named_parameters() order
    assert len(names) == len(opt["state"]) and all(tuple(opt["state"][i]["exp_avg_sq"].shape) == tuple(hip[k].shape) for i, k in enumerate(names))
    steps = int(float(opt["state"][0]["step"]))
    gate = 0.01 * steps * 1e-4
    kept = total = 0
    for i, k in enumerate(names):
        diff = (hip[k].double() - ref[k].double()).abs()
        rms = opt["state"][i]["exp_avg_sq"].double().sqrt()
        signal = rms >= 1e-3 * rms.max()
        d = float(diff[signal].max())
        d_noise = float(diff[~signal].max()) if bool((~signal).any()) else 0.0
        print(f"{k}: hip against torch {d:.3e} on {int(signal.sum())} of {signal.numel()} elements (gate {gate:.3e}); {d_noise:.3e} on the rest (not asserted)")
        assert int(signal.sum()) >= 0.25 * signal.numel(), (k, int(signal.sum()), signal.numel())
        assert d <= gate, (k, d, gate)
        kept, total = kept + int(signal.sum()), total + signal.numel()
    assert kept >= 0.9 * total, (kept, total)
    for k in hip:
        if k not in names:
            assert torch.equal(hip[k], ref[k]), k
