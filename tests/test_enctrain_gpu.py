"""The SegmentEncoder training step (libtamf_enctrain.so, SegmentEncoderTrainStep) on the MI355X: the reference's loss and gradients
(tests/golden/enctrain_*.npz) inside the gate measured on the reference itself, the float64 restatement over a shape sweep, dropout
with the library's own masks injected into the restatement, determinism and batch invariance bit for bit, a short SGD run against
the reference's loss curve, and the refusals.

Gates.  A fixture's gate is its tol_rel / tol_rel_loss (4 x the reference's own float32-against-float64 error), and the dropout
cases run on fixtures' weights and inputs against those same stored gates.  A sweep case has no reference run, so its gate is
measured the same way at test time - 4 x the error of the restatement run in float32 against the restatement in float64 (per case:
max over tensors of |g32 - g64|_inf / |g64|_inf, and the loss) - and the gradient gate is capped at the largest fixture gate
(FIXTURE_TOL_MAX), so that no sweep case is held to less than the fixtures are; both are printed.  One float32 run's
loss can land on the float32 nearest the float64 value by luck, which no other summation order can be asked to repeat: the loss is
returned as ONE float32, whose rounding alone is up to 2^-24 relative, so a measured loss error below 2^-24 counts as 2^-24."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from encoder_restatement import ARCH_ENCODER, seeded_inputs, seeded_state_dict  # noqa: E402
from encoder_train_restatement import BUFFERS, grad_rel_err, load_train_case, loss_and_grads, site_shapes  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")
FIXTURES = ("enctrain_small_ragged.npz", "enctrain_l1_ff16.npz", "enctrain_nonfinite.npz", "enctrain_full_arch.npz", "enctrain_sgd.npz")
SMALL = dict(ARCH_ENCODER, obj_embed_dim=32)
FIXTURE_TOL_MAX = max(float(np.load(os.path.join(GOLDEN, f))["tol_rel"]) for f in FIXTURES)


def _model(arch, sd):
    import torch

    from oakink2_tamf_amd.model.segment_encoder import SegmentEncoder

    m = SegmentEncoder(17, **arch).to("cuda:0")
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    return m


def _batch(inputs, rows=None):
    import torch

    sl = slice(None) if rows is None else rows
    b = {k: torch.from_numpy(np.ascontiguousarray(inputs[k][sl])).to("cuda:0") for k in ("pose_repr", "shape", "obj_embedding", "obj_traj")}
    b["hand_side"] = [inputs["hand_side"][i] for i in (range(len(inputs["hand_side"])) if rows is None else rows)]
    return b


def _step(arch, sd, B, T, p=0.0, seed=0):
    from oakink2_tamf_amd.model.segment_encoder_train import SegmentEncoderTrainStep

    m = _model(arch, sd)
    return m, SegmentEncoderTrainStep(m, B, T, dropout=p, seed=seed)


def _run(m, ts, inputs, labels, obj_num=None, clip_ids=None, step=0, rows=None):
    """one call with every gradient buffer pre-filled with NaN -> (loss, activation, {key: gradient}) as numpy"""
    import torch

    for p_ in m.parameters():
        p_.grad.fill_(float("nan"))
    lab = np.asarray(labels)[rows] if rows is not None else np.asarray(labels)
    out = ts.loss_and_grads(_batch(inputs, rows), lab, obj_num=obj_num, clip_ids=clip_ids, step=step)
    torch.cuda.synchronize()
    grads = {k: v.grad.cpu().numpy().copy() for k, v in m.named_parameters()}
    return float(out["loss"].cpu()), out["activation"].cpu().numpy().copy(), grads


def _gate32(sd, arch, inputs, labels, obj_num, ref, masks=None, p=0.0):
    """4 x the float32 restatement's error against the float64 one `ref` = (loss, act, grads)"""
    import torch

    l32, _, g32 = loss_and_grads(sd, arch, inputs, labels, obj_num, masks, p, dtype=torch.float32)
    measured = 4 * max(grad_rel_err(g32, ref[2]).values())
    print(f"gate measured at test time {measured:.3e}, largest fixture gate {FIXTURE_TOL_MAX:.3e}")
    return min(measured, FIXTURE_TOL_MAX), 4 * max(abs(l32 - ref[0]) / abs(ref[0]), 2.0 ** -24)


def _check(tag, got, ref, tol, tol_loss):
    loss, _, grads = got
    assert set(grads) == set(ref[2]) and not set(grads) & set(BUFFERS)
    err = grad_rel_err(grads, ref[2])
    worst = max(err, key=err.get)
    eloss = abs(loss - ref[0]) / abs(ref[0])
    print(f"{tag}: loss {loss:.8f} ref {ref[0]:.8f} rel {eloss:.3e} (gate {tol_loss:.3e}); worst gradient {worst} rel {err[worst]:.3e} (gate {tol:.3e})")
    assert err[worst] <= tol, (tag, worst, err[worst], tol)
    assert eloss <= tol_loss, (tag, loss, ref[0], eloss, tol_loss)


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixture(name):
    """loss and every gradient of the reference's own module and loss, inside 4 x the reference's float32 error; every gradient element
    written (the buffers start as NaN; NaN stays only where torch's own gradient is NaN).
    Measured on the MI355X: see the figures in DESIGN.md section 4."""
    c = load_train_case(os.path.join(GOLDEN, name))
    B, T = c["inputs"]["pose_repr"].shape[:2]
    m, ts = _step(c["arch"], c["sd"], B, T)
    got = _run(m, ts, c["inputs"], c["labels"], c["obj_num"])
    _check(name, got, (c["loss"], None, c["grads"]), c["tol_rel"], c["tol_rel_loss"])
    ts.close()
    m.close()


def _case(seed, arch, B, T, nobj, obj_num=None):
    sd = seeded_state_dict(arch, seed)
    inp = seeded_inputs(B, T, nobj, seed + 1, obj_num=obj_num, arch=arch)
    inp["hand_side"] = ["lh" if (b + seed) % 2 else "rh" for b in range(B)]
    F = arch["input_dim"]
    labels = np.random.default_rng(seed + 2).integers(0, F, B)
    labels[0] = 0 if seed % 2 else F - 1
    labels[-1] = F - 1 if seed % 2 else 0
    return sd, inp, labels


SWEEP = [  # (T, B, num_layers, ff_size, nobj, obj_num): S = T + 4 below a tile, a partial tile, 16, 32, across 64 + 4 and 160 frames
    (1, 1, 1, 16, 1, None), (1, 3, 2, 128, 3, [3, 1, 2]), (7, 3, 1, 128, 3, None), (7, 1, 3, 16, 1, [1]), (12, 3, 2, 16, 3, [2, 3, 1]),
    (12, 1, 1, 128, 3, None), (28, 3, 3, 128, 1, None), (28, 1, 2, 16, 3, [2]), (61, 3, 2, 128, 3, [1, 2, 3]), (61, 1, 1, 16, 1, None),
    (160, 3, 2, 128, 3, [3, 3, 1]), (160, 1, 3, 16, 3, None),
]


@pytest.mark.parametrize("T,B,L,ff,nobj,obj_num", SWEEP)
def test_restatement_sweep(T, B, L, ff, nobj, obj_num):
    arch = dict(SMALL, num_layers=L, ff_size=ff)
    sd, inp, labels = _case(1000 + 7 * T + B + L, arch, B, T, nobj, obj_num)
    ref = loss_and_grads(sd, arch, inp, labels, obj_num)
    tol, tol_loss = _gate32(sd, arch, inp, labels, obj_num, ref)
    m, ts = _step(arch, sd, B, T)
    got = _run(m, ts, inp, labels, obj_num)
    _check(f"T{T} B{B} L{L} ff{ff}", got, ref, tol, tol_loss)
    # the training forward at p = 0 computes the inference kernel's activation (uncomposed against composed input maps)
    act = m.encode(_batch(inp), obj_num=obj_num)["activation"].cpu().numpy()
    assert np.abs(got[1] - act).max() <= 2e-5 * np.abs(act).max(), (np.abs(got[1] - act).max(), np.abs(act).max())
    ts.close()
    m.close()


def test_same_call_same_bits():
    arch = dict(SMALL)
    sd, inp, labels = _case(2001, arch, 3, 28, 2)
    for p in (0.0, 0.1):
        m, ts = _step(arch, sd, 3, 28, p=p, seed=5)
        a = _run(m, ts, inp, labels, step=3)
        b = _run(m, ts, inp, labels, step=3)
        assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes() and a[1].tobytes() == b[1].tobytes()
        for k in a[2]:
            assert a[2][k].tobytes() == b[2][k].tobytes(), (p, k)
        ts.close()


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_clip_activation_is_batch_invariant(p):
    """a clip's activation: alone, in a batch of 5, and at another position with its clip id kept"""
    arch = dict(SMALL)
    sd, inp, labels = _case(2101, arch, 5, 12, 2)
    m, ts = _step(arch, sd, 5, 12, p=p, seed=9)
    ids = [40, 41, 42, 43, 44]
    full = _run(m, ts, inp, labels, clip_ids=ids)[1]
    alone = _run(m, ts, inp, labels, clip_ids=[42], rows=[2])[1]
    moved = _run(m, ts, inp, labels, clip_ids=[44, 42, 40], rows=[4, 2, 0])[1]
    assert full[2].tobytes() == alone[0].tobytes() == moved[1].tobytes()
    if p > 0:  # the key is the clip id, not the position: another id gives another mask
        other = _run(m, ts, inp, labels, clip_ids=[7], rows=[2])[1]
        assert other[0].tobytes() != alone[0].tobytes()
    ts.close()


def _masks(arch, T, p, seed, step, clip_ids):
    from oakink2_tamf_amd.model.segment_encoder_train import dropout_mask

    return {site: np.stack([dropout_mask(seed, step, c, site, r, k, p).cpu().numpy() for c in clip_ids], 0)
            for site, (r, k) in site_shapes(arch, T).items()}


@pytest.mark.parametrize("name", ["enctrain_small_ragged.npz", "enctrain_l1_ff16.npz"])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_with_injected_masks(name, p):
    """a fixture's weights, inputs and labels with dropout on: the masks of tamf_enctrain_dropout_mask injected into the restatement,
    loss and gradients inside that fixture's stored gate (4 x the reference's own float32 error on these weights and inputs)"""
    c = load_train_case(os.path.join(GOLDEN, name))
    B, T = c["inputs"]["pose_repr"].shape[:2]
    ids, seed, step = [11 + 6 * b for b in range(B)], 77, 4
    masks = _masks(c["arch"], T, p, seed, step, ids)
    assert all(0 < mk.mean() < 1 for mk in masks.values())  # (every site really drops something)
    ref = loss_and_grads(c["sd"], c["arch"], c["inputs"], c["labels"], c["obj_num"], masks, p)
    m, ts = _step(c["arch"], c["sd"], B, T, p=p, seed=seed)
    got = _run(m, ts, c["inputs"], c["labels"], c["obj_num"], clip_ids=ids, step=step)
    ts.close()
    m.close()
    _check(f"{name} p{p}", got, ref, c["tol_rel"], c["tol_rel_loss"])


def test_p0_gives_the_bits_of_every_mask_forced_to_keep():
    """p = 2^-32 puts the keep threshold at 1: the step goes through the Philox draw of every element and keeps all of them (a draw
    of exactly 0 has probability 2^-32 per element; the masks are checked), and 1 / (1 - p) rounds to exactly 1.0f.  p = 0 skips
    the draw.  Loss, activation and every gradient have to be the same bits."""
    arch = dict(SMALL)
    B, T, obj_num, ids, seed, step = 3, 12, [2, 1, 2], [3, 1 << 33, 9], 21, 6
    sd, inp, labels = _case(2401, arch, B, T, 2, obj_num)
    p = 2.0 ** -32
    masks = _masks(arch, T, p, seed, step, ids)
    assert all(mk.all() for mk in masks.values())
    out = []
    for prob in (0.0, p):
        m, ts = _step(arch, sd, B, T, p=prob, seed=seed)
        out.append(_run(m, ts, inp, labels, obj_num, clip_ids=ids, step=step))
        ts.close()
        m.close()
    (l0, a0, g0), (l1, a1, g1) = out
    assert np.float32(l0).tobytes() == np.float32(l1).tobytes() and a0.tobytes() == a1.tobytes()
    for k in g0:
        assert g0[k].tobytes() == g1[k].tobytes(), k


def test_zero_grad_between_steps_keeps_training():
    """optimizer.zero_grad() sets .grad to None by default: the next step has to write gradients the optimiser sees"""
    import torch

    arch = dict(SMALL, num_layers=1, ff_size=16)
    sd, inp, labels = _case(2501, arch, 2, 7, 1)
    m, ts = _step(arch, sd, 2, 7)
    opt = torch.optim.SGD(m.parameters(), lr=1e-2)
    batch = _batch(inp)
    ts.loss_and_grads(batch, labels)
    first = {k: v.grad.clone() for k, v in m.named_parameters()}
    opt.zero_grad()
    assert all(v.grad is None for v in m.parameters())
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    ts.loss_and_grads(batch, labels)
    for k, v in m.named_parameters():
        assert v.grad is not None and torch.equal(v.grad, first[k]), k
    opt.step()
    assert all(not torch.equal(v.detach(), before[k]) for k, v in m.named_parameters())
    for v in m.parameters():  # a gradient tensor assigned by the caller is bound where it is
        v.grad = torch.full_like(v, float("nan"))
    ts.loss_and_grads(batch, labels)
    torch.cuda.synchronize()
    assert all(torch.isfinite(v.grad).all() for v in m.parameters())
    ts.close()
    m.close()


def test_dropout_mask_statistics_and_keys():
    from oakink2_tamf_amd.model.segment_encoder_train import dropout_mask

    rows, cols = 400, 256  # 102 400 elements
    n = rows * cols
    for p in (0.1, 0.5):
        kept = float(dropout_mask(3, 0, 0, 0, rows, cols, p).float().sum().cpu())
        sd = (n * p * (1 - p)) ** 0.5
        assert abs(kept - n * (1 - p)) <= 5 * sd, (p, kept, n * (1 - p), sd)
    base = dropout_mask(3, 1, 2, 4, rows, cols, 0.5).cpu().numpy()
    assert (dropout_mask(3, 1, 2, 4, rows, cols, 0.5).cpu().numpy() == base).all()
    for other in ((4, 1, 2, 4), (3, 2, 2, 4), (3, 1, 3, 4), (3, 1, 2, 5), (3, 1, 2 + (1 << 32), 4), (3 + (1 << 32), 1, 2, 4)):
        diff = (dropout_mask(*other, rows, cols, 0.5).cpu().numpy() != base).mean()
        assert 0.45 < diff < 0.55, (other, diff)  # (independent masks differ in half of the elements; 5 sd of that is 0.008)
    assert dropout_mask(3, 1, 2, 4, rows, cols, 0.0).all()


def test_sgd_run_follows_reference_curve():
    """10 plain-SGD steps through SegmentEncoderTrainStep + torch.optim.SGD against the reference's float64 loss curve, inside 4 x the
    deviation of the reference's own float32 run"""
    import torch

    c = load_train_case(os.path.join(GOLDEN, "enctrain_sgd.npz"))
    B, T = c["inputs"]["pose_repr"].shape[:2]
    m, ts = _step(c["arch"], c["sd"], B, T)
    opt = torch.optim.SGD(m.parameters(), lr=float(c["sgd_lr"]))
    batch = _batch(c["inputs"])
    curve = []
    for _ in range(len(c["sgd_loss"])):
        curve.append(float(ts.loss_and_grads(batch, c["labels"])["loss"].cpu()))
        opt.step()
    dev = np.abs(np.array(curve) - c["sgd_loss"])
    print("sgd curve", curve, "deviation", dev.max(), "gate", 4 * float(c["sgd_dev32"]))
    assert dev.max() <= 4 * float(c["sgd_dev32"]), (dev, float(c["sgd_dev32"]))
    m.refresh_hip_weights()  # the inference path sees the trained weights
    act = m.encode(batch)["activation"]
    out = ts.loss_and_grads(batch, c["labels"])
    assert (out["activation"] - act).abs().max() <= 2e-5 * act.abs().max()
    ts.close()
    m.close()


def test_refusals():
    import torch

    from oakink2_tamf_amd.hip_backend import TamfError
    from oakink2_tamf_amd.model.segment_encoder_train import SegmentEncoderTrainStep

    arch = dict(SMALL, num_layers=1, ff_size=16)
    sd, inp, labels = _case(2301, arch, 2, 7, 1)
    m = _model(arch, sd)
    with pytest.raises(TamfError, match="max_frames"):
        SegmentEncoderTrainStep(m, 2, 509)
    for bad, word in ((dict(arch, ff_size=24), "ff_size"), (dict(arch, ff_size=528), "ff_size"), (dict(arch, latent_dim=128, num_heads=4), "latent_dim"),
                      (dict(arch, num_heads=8), "heads")):
        mb = _model(bad, seeded_state_dict(bad, 1))
        with pytest.raises(TamfError, match=word):
            SegmentEncoderTrainStep(mb, 2, 7)
        mb.close()

    def nan_grads(model):
        for v in model.parameters():
            v.grad.fill_(float("nan"))

    def untouched(model):  # nothing was launched: every gradient element is still the NaN it was filled with
        torch.cuda.synchronize()
        return all(bool(torch.isnan(v.grad).all()) for v in model.parameters())

    ts = SegmentEncoderTrainStep(m, 1, 7)
    nan_grads(m)
    with pytest.raises(TamfError, match="max_batch"):
        ts.loss_and_grads(_batch(inp), labels)
    with pytest.raises(ValueError):
        ts.loss_and_grads(_batch(inp, [0]), [arch["input_dim"]])
    assert untouched(m)
    ts.close()
    m.close()
    m2 = _model(arch, sd)
    ts2 = _UnboundStep(m2, 2, 7)
    nan_grads(m2)
    with pytest.raises(TamfError, match="missing binding 'input_merge.2.bias'"):
        ts2.loss_and_grads(_batch(inp), labels)
    assert untouched(m2)
    ts2.close()
    m2.close()


class _UnboundStep:
    """SegmentEncoderTrainStep whose first bind leaves 'input_merge.2.bias' out"""

    def __new__(cls, model, max_batch, max_frames):
        from oakink2_tamf_amd.model.segment_encoder_train import SegmentEncoderTrainStep

        class Step(SegmentEncoderTrainStep):
            def bind(self, skip=()):
                super().bind(skip=("input_merge.2.bias",))

        return Step(model, max_batch, max_frames)


def test_train_encoder_launcher_end_to_end(tmp_path):
    """2 epochs of launch/train_encoder.py on a synthetic cache (AdamW, clipping, the schedule): both checkpoints are written, the
    model file loads into SegmentEncoder as it is, and compute_score_fid runs with it"""
    import json
    import subprocess

    import torch

    from enctrain_fixture import ROOT, launcher_cmd, launcher_env, write_training_tree
    from oakink2_tamf_amd.model.segment_encoder import SegmentEncoder

    paths, n = write_training_tree(str(tmp_path), n_segments=8)
    cmd = launcher_cmd(paths, "--train.batch_size", "8", "--train.num_epoch", "2", "--train.scheduler_milestone", "1", "--train.record_freq", "20",
                        "--val.val_freq", "1", "--runtime.seed", "3", "--exp_id", "e2e", "--commit")
    r = subprocess.run(cmd, capture_output=True, text=True, env=launcher_env(), cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    save = os.path.join(str(tmp_path), "common", "train_encoder", "e2e", "save")
    assert sorted(os.listdir(save)) == ["model_0000.pt", "model_0001.pt", "optimizer_0000.pt", "optimizer_0001.pt"]
    assert "val epoch 0001" in r.stderr + r.stdout and "lr [5e-05]" in r.stderr + r.stdout
    state = torch.load(os.path.join(save, "model_0001.pt"), map_location="cpu")
    first = torch.load(os.path.join(save, "model_0000.pt"), map_location="cpu")
    model = SegmentEncoder(69, **dict(ARCH_ENCODER))
    missing, unexpected = model.load_state_dict(state, strict=True)
    assert not missing and not unexpected
    assert all(torch.isfinite(v).all() for v in state.values())
    assert any(not torch.equal(state[k], first[k]) for k in state)  # the second epoch moved the weights
    opt = torch.load(os.path.join(save, "optimizer_0001.pt"), map_location="cpu")
    assert opt["param_groups"][0]["lr"] == pytest.approx(5e-5) and len(opt["state"]) == len(list(model.parameters()))

    # compute_score_fid with the trained checkpoint: the generated set is the ground truth itself here
    from oakink2_tamf_amd.dataset.interaction_segment import InteractionSegmentData, load_cache_dict
    from oakink2_tamf_amd.launch import formats

    ds = InteractionSegmentData(obj_embedding_prefix=paths["emb"], obj_pointcloud_prefix=paths["pc"], cache_dict=load_cache_dict(paths["cache"]))
    tree = os.path.join(str(tmp_path), "srf")
    rng = np.random.default_rng(5)
    for i in range(len(ds)):
        it = ds[i]
        T = it["pose_repr"].shape[0]
        pose = (it["pose_repr"] + 0.2 * rng.normal(size=it["pose_repr"].shape)).astype(np.float32)
        d = formats.build_refine_save_dict(it["info"], it["hand_side"], np.zeros((T, 21, 3)), np.zeros((T, 778, 3)), None, it["obj_list"],
                                           int(it["len"]), it["frame_id"], pose)
        path = formats.refine_sample_path_in(tree, it["info"])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            import pickle

            pickle.dump(d, f)
    out_json = os.path.join(str(tmp_path), "fid.json")
    cmd = [sys.executable, "-m", "oakink2_tamf_amd.launch.compute_score_fid", "--cfg", os.path.join(ROOT, "config", "arch_encoder.yml"),
           "--debug.cache_dict_filepath", paths["cache"], "--data.obj_embedding_prefix", paths["emb"], "--data.obj_pointcloud_prefix", paths["pc"],
           "--debug.sample_refine_filepath", tree, "--debug.encoder_checkpoint_filepath", os.path.join(save, "model_0001.pt"), "--out_json", out_json]
    r = subprocess.run(cmd, capture_output=True, text=True, env=launcher_env(), timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(out_json) as f:
        terms = json.load(f)
    assert terms["n_clips"] >= 2 and all(np.isfinite(v) for k, v in terms.items() if k != "n_clips"), terms
