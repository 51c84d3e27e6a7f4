"""The denoiser's training step (libtamf_mdmtrain.so, InterationSegmentMDMTrainStep) on the MI355X, at head dimensions 64 and 128: the
reference's output and gradients (tests/golden/mdmtrain_*.npz) inside the gates measured on the reference itself, float64 autograd
through oracle.mdm_oracle.denoiser_forward over a shape sweep and on the two shipped configurations, non-finite inputs, dropout with
the library's own masks injected into the float64 restatement, determinism and batch invariance bit for bit, the inference path on the
same weights, the reference's training_losses terms and its SGD loss curve, and the refusals.

Gates.  A fixture's gates are its tol_rel (gradients) and tol_rel_out (output): 4 x the reference's own float32-against-float64 error;
the dropout cases run on fixtures' weights and inputs against those same stored gates.  A sweep case has no reference run, so its gates
are measured the same way at test time - 4 x the error of the oracle's float32 autograd against its float64 autograd (max over
tensors of |g32 - g64|_inf / |g64|_inf, and the same for the output) - capped at the largest fixture gate; both are printed."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mdm_train_restatement as M  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")
FIXTURES = ("mdmtrain_l1_hd64.npz", "mdmtrain_l1_hd128.npz", "mdmtrain_tiny_hd64.npz", "mdmtrain_tiny_hd128.npz")
_TOLS = [np.load(os.path.join(GOLDEN, f)) for f in FIXTURES + ("mdmtrain_losses.npz",)]
FIXTURE_TOL_MAX, FIXTURE_TOL_OUT_MAX = max(float(z["tol_rel"]) for z in _TOLS), max(float(z["tol_rel_out"]) for z in _TOLS)
ARCHS = {"l1_64": M.ARCH_L1_64, "l1_128": M.ARCH_L1_128, "tiny_64": M.ARCH_TINY_64, "tiny_128": M.ARCH_TINY_128}
BATCH_KEYS = ("text_embedding", "shape", "obj_embedding", "obj_traj")


def _model(arch, sd, p=0.0):
    from oakink2_tamf_amd.model.interaction_segment_mdm import InterationSegmentMDM

    m = InterationSegmentMDM(**M.arch_dict(arch), dropout=p, precision="f32").to("cuda:0")
    m.load_state_dict(M.module_state_dict(sd))
    return m


def _batch(inp, rows=None):
    """-> (x_t, t, batch) on the device"""
    import torch

    sl = slice(None) if rows is None else rows
    b = {k: torch.from_numpy(np.ascontiguousarray(inp[k][sl])).to("cuda:0") for k in BATCH_KEYS}
    b["hand_side"] = [inp["hand_side"][i] for i in (range(len(inp["hand_side"])) if rows is None else rows)]
    return torch.from_numpy(np.ascontiguousarray(inp["x_t"][sl])).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(np.asarray(inp["t"])[sl])), b


def _step(arch, sd, B, T, p=0.0, seed=0):
    from oakink2_tamf_amd.model.interaction_segment_mdm_train import InterationSegmentMDMTrainStep

    m = _model(arch, sd, p)
    return m, InterationSegmentMDMTrainStep(m, B, T, dropout=p, seed=seed)


def _grads(m):
    return {k: v.grad.cpu().numpy().copy() for k, v in m.named_parameters()}


def _run(m, ts, inp, G, obj_num=None, clip_ids=None, step=0, rows=None):
    """one forward + backward of loss = sum(G * out), every gradient buffer pre-filled with NaN -> (out, {key: gradient}) as numpy"""
    import torch

    for p_ in m.parameters():
        p_.grad.fill_(float("nan"))
    out = ts.forward(*_batch(inp, rows), obj_num=obj_num, clip_ids=clip_ids, step=step)
    g = torch.from_numpy(np.ascontiguousarray(np.asarray(G, np.float32)[slice(None) if rows is None else rows])).to("cuda:0")
    (out * g).sum().backward()
    torch.cuda.synchronize()
    return out.detach().cpu().numpy().copy(), _grads(m)


def _masks(ts, arch, B, T, step=0, clip_ids=None):
    import torch

    return {s: torch.stack([ts.dropout_mask(step, b if clip_ids is None else clip_ids[b], s, r, c) for b in range(B)]).cpu()
            for s, (r, c) in M.site_shapes(arch, T).items()}


def _check(tag, got, ref, tol, tol_out):
    out, grads = got
    assert set(grads) == set(ref[2]) and not set(grads) & set(M.BUFFERS)
    err = M.grad_rel_err(grads, ref[2])
    worst = max(err, key=err.get)
    e_out = M.rel_err(out, ref[0])
    print(f"{tag}: output rel {e_out:.3e} (gate {tol_out:.3e}); worst gradient {worst} rel {err[worst]:.3e} (gate {tol:.3e})")
    assert e_out <= tol_out, (tag, e_out, tol_out)
    assert err[worst] <= tol, (tag, worst, err[worst], tol)


def _shape(c):
    B, _, _, T = c["inputs"]["x_t"].shape
    return B, T


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixture(name):
    """output and every gradient of the reference's own module inside 4 x the reference's float32 error; every gradient element
    written (the buffers start as NaN)"""
    c = M.load_case(os.path.join(GOLDEN, name))
    B, T = _shape(c)
    m, ts = _step(c["arch"], c["sd"], B, T)
    out, grads = _run(m, ts, c["inputs"], c["G"], c["obj_num"])
    assert not any(np.isnan(g).any() for g in grads.values())
    err = M.fixture_grad_err(grads, c)
    worst = max(err, key=err.get)
    e_out = M.rel_err(out, c["out"])
    loss = float((c["G"].astype(np.float64) * out.astype(np.float64)).sum())
    print(f"{name}: output rel {e_out:.3e} (gate {c['tol_rel_out']:.3e}); worst gradient {worst} rel {err[worst]:.3e} (gate {c['tol_rel']:.3e}); "
          f"loss rel {abs(loss - c['loss']) / abs(c['loss']):.3e}")
    assert e_out <= c["tol_rel_out"]
    assert err[worst] <= c["tol_rel"], (worst, err[worst])
    ts.close()


def _sweep_case(arch, B, T, ragged, seed):
    sd = M.seeded_state_dict(arch, seed)
    inp, obj_num = M.seeded_inputs(arch, B, T, 2, seed + 1, ragged)
    G = np.random.default_rng(seed + 2).normal(size=(B, arch.input_dim, 1, T)).astype(np.float32)
    return sd, inp, obj_num, G


def _oracle_gates(sd, arch, inp, G, obj_num):
    """float64 autograd through the oracle, and the gates 4 x (the oracle's float32 autograd against it), capped at the fixtures'"""
    import torch

    ref = M.loss_and_grads(sd, arch, inp, G, obj_num, forward=M.oracle_forward)
    r32 = M.loss_and_grads(sd, arch, inp, G, obj_num, dtype=torch.float32, forward=M.oracle_forward)
    m_g, m_o = 4 * max(M.grad_rel_err(r32[2], ref[2]).values()), 4 * M.rel_err(r32[0], ref[0])
    print(f"gates measured at test time: gradients {m_g:.3e} (largest fixture gate {FIXTURE_TOL_MAX:.3e}), output {m_o:.3e} ({FIXTURE_TOL_OUT_MAX:.3e})")
    return ref, min(m_g, FIXTURE_TOL_MAX), min(m_o, FIXTURE_TOL_OUT_MAX)


@pytest.mark.parametrize("ragged", [False, True], ids=["padded", "ragged"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 11, 12, 59, 60, 191])  # S = 6, 16, 17, 64, 65, 196: below, at and across the 16-row and 64-row tiles
@pytest.mark.parametrize("arch_name", sorted(ARCHS))
def test_sweep_against_oracle_autograd(arch_name, T, B, ragged):
    arch = ARCHS[arch_name]
    sd, inp, obj_num, G = _sweep_case(arch, B, T, ragged, 1000 + 7 * T + B)
    ref, tol, tol_out = _oracle_gates(sd, arch, inp, G, obj_num)
    m, ts = _step(arch, sd, B, T)
    _check(f"{arch_name} T{T} B{B} {'ragged' if ragged else 'padded'}", _run(m, ts, inp, G, obj_num), ref, tol, tol_out)
    ts.close()


@pytest.mark.parametrize("config,expect", [("arch_mdm_l.yml", (512, 4, 2048, 8)), ("arch_mdm.yml", (256, 4, 1024, 8))])
def test_full_configuration_against_oracle_autograd(config, expect):
    """config/arch_mdm_l.yml itself (latent 512, 4 heads: head dimension 128; ff 2048, 8 layers, 768-wide object embeddings, clip_dim
    512) and config/arch_mdm.yml (latent 256: head dimension 64) at B 2, T 11, ragged"""
    import yaml

    with open(os.path.join(HERE, "..", "config", config)) as f:
        cfg = yaml.safe_load(f)["model"]
    arch = M.mo.Arch(kind="G", **{k: int(cfg[k]) for k in M.ARCH_NAMES if k in cfg})
    assert (arch.latent_dim, arch.num_heads, arch.ff_size, arch.num_layers) == expect and (arch.obj_embed_dim, arch.clip_dim) == (768, 512)
    sd, inp, obj_num, G = _sweep_case(arch, 2, 11, True, 3000)
    ref, tol, tol_out = _oracle_gates(sd, arch, inp, G, obj_num)
    m, ts = _step(arch, sd, 2, 11)
    _check(f"{config} T11 B2", _run(m, ts, inp, G, obj_num), ref, tol, tol_out)
    ts.close()


def test_nonfinite_inputs():
    """NaN in one clip's obj_embedding and in one text_embedding element: the nan_to_num of the prefix rows passes gradient where its
    input is finite - the gradients equal the float64 autograd's where those are finite and are NaN where they are NaN (0 * NaN in the
    weight gradients behind the mask)"""
    arch = M.ARCH_TINY_128
    sd, inp, obj_num, G = _sweep_case(arch, 3, 12, False, 4000)
    inp["obj_embedding"][1, 0, 3] = np.nan
    inp["text_embedding"][2, 5] = np.nan
    ref, tol, tol_out = _oracle_gates(sd, arch, inp, G, obj_num)
    assert any(np.isnan(g).any() for g in ref[2].values()) and not all(np.isnan(g).all() for g in ref[2].values())
    m, ts = _step(arch, sd, 3, 12)
    _check("nonfinite", _run(m, ts, inp, G, obj_num), ref, tol, tol_out)
    ts.close()


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name", ["mdmtrain_tiny_hd64.npz", "mdmtrain_tiny_hd128.npz"])
def test_dropout_with_the_librarys_masks(name, p):
    """the library's own keep-masks (dropout_mask) injected into the float64 restatement; the fixture's gates"""
    c = M.load_case(os.path.join(GOLDEN, name))
    B, T = _shape(c)
    m, ts = _step(c["arch"], c["sd"], B, T, p=p, seed=77)
    clip_ids = [5 + 3 * b for b in range(B)]
    got = _run(m, ts, c["inputs"], c["G"], c["obj_num"], clip_ids=clip_ids, step=4)
    masks = _masks(ts, c["arch"], B, T, step=4, clip_ids=clip_ids)
    kept = np.mean([float(v.float().mean()) for v in masks.values()])
    assert abs(kept - (1 - p)) < 0.05
    ref = M.loss_and_grads(c["sd"], c["arch"], c["inputs"], c["G"], c["obj_num"], masks, p)
    _check(f"{name} p={p}", got, ref, c["tol_rel"], c["tol_rel_out"])
    ts.close()


def test_tiny_p_gives_the_bits_of_no_dropout():
    """p = 2^-32: the threshold is 1, every draw keeps (none of these draws is 0) and the scale rounds to 1 - the bits of p = 0"""
    c = M.load_case(os.path.join(GOLDEN, "mdmtrain_tiny_hd128.npz"))
    B, T = _shape(c)
    m0, ts0 = _step(c["arch"], c["sd"], B, T, p=0.0)
    m1, ts1 = _step(c["arch"], c["sd"], B, T, p=2.0 ** -32)
    a, b = _run(m0, ts0, c["inputs"], c["G"], c["obj_num"]), _run(m1, ts1, c["inputs"], c["G"], c["obj_num"])
    assert all(bool(v.all()) for v in _masks(ts1, c["arch"], B, T).values())
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])
    ts0.close()
    ts1.close()


@pytest.mark.parametrize("arch_name", ["tiny_64", "tiny_128"])
def test_clip_invariance_and_determinism(arch_name):
    """with obj_num given, a clip's forward has the same bits alone and at another batch position under the same clip id, and other
    bits under another id; the same forward + backward twice gives identical bits in every gradient, overwritten, not accumulated"""
    import torch

    arch = ARCHS[arch_name]
    sd, inp, obj_num, G = _sweep_case(arch, 3, 12, True, 5000)
    m, ts = _step(arch, sd, 3, 12, p=0.3, seed=11)
    ids = [40, 41, 42]
    full, g1 = _run(m, ts, inp, G, obj_num, clip_ids=ids, step=2)
    full2, g2 = _run(m, ts, inp, G, obj_num, clip_ids=ids, step=2)  # (the gradient buffers were NaN again before this call)
    assert np.array_equal(full, full2) and all(np.array_equal(g1[k], g2[k]) for k in g1)
    assert not any(np.isnan(g).any() for g in g2.values())
    with torch.no_grad():
        alone = ts.forward(*_batch(inp, [1]), obj_num=[obj_num[1]], clip_ids=[41], step=2).cpu().numpy()
        ts.discard_forward()
        moved = ts.forward(*_batch(inp, [2, 1]), obj_num=[obj_num[2], obj_num[1]], clip_ids=[42, 41], step=2).cpu().numpy()
        ts.discard_forward()
        other = ts.forward(*_batch(inp, [1]), obj_num=[obj_num[1]], clip_ids=[43], step=2).cpu().numpy()
        ts.discard_forward()
    assert np.array_equal(alone[0], full[1]) and np.array_equal(moved[1], full[1]) and np.array_equal(moved[0], full[2])
    assert not np.array_equal(other[0], full[1])
    ts.close()


@pytest.mark.parametrize("name", ["mdmtrain_tiny_hd64.npz", "mdmtrain_tiny_hd128.npz"])
def test_forward_agrees_with_the_inference_path(name):
    """p = 0: the training forward against InterationSegmentMDM(precision="f32") on the same weights, inside the fixture's output gate"""
    import torch

    c = M.load_case(os.path.join(GOLDEN, name))
    B, T = _shape(c)
    m, ts = _step(c["arch"], c["sd"], B, T)
    x, t, batch = _batch(c["inputs"])
    with torch.no_grad():
        a = ts.forward(x, t, batch).cpu().numpy()  # (padded object means: the reference's forward on the batch it is given)
        ts.discard_forward()
        b = m(x, t.to("cuda:0"), batch).cpu().numpy()
    e = float(np.abs(a - b).max() / np.abs(b).max())
    print(f"training forward against the inference path: rel {e:.3e} (gate {c['tol_rel_out']:.3e})")
    assert e <= c["tol_rel_out"]
    ts.close()


def _objective(name):
    import torch

    sys.path.insert(0, os.path.join(HERE, "..", "oakink2-tamf_amd"))
    from oakink2_tamf_amd.model.diffusion_util import create_gaussian_diffusion

    c = M.load_case(os.path.join(GOLDEN, name))
    inp = c["inputs"]
    batch = {k: torch.from_numpy(np.ascontiguousarray(inp[k])) for k in BATCH_KEYS}
    batch["hand_side"], batch["mask"] = inp["hand_side"], torch.from_numpy(inp["mask"])
    batch["pose_repr"] = torch.from_numpy(np.ascontiguousarray(inp["x_start"][:, :, 0, :].transpose(0, 2, 1)))
    return c, create_gaussian_diffusion(int(c["z"]["diffusion_steps"]), "cosine"), batch


def test_training_losses_through_the_step():
    """loss_and_grads on mdmtrain_losses.npz: the reference's mse per clip, its loss and every gradient inside that file's gates"""
    import torch

    c, diffusion, batch = _objective("mdmtrain_losses.npz")
    z, inp = c["z"], c["inputs"]
    B, T = inp["x_start"].shape[0], inp["x_start"].shape[3]
    m, ts = _step(c["arch"], c["sd"], B, T)
    for p_ in m.parameters():
        p_.grad.fill_(float("nan"))
    res = ts.loss_and_grads(diffusion, batch, t=torch.from_numpy(inp["t"]), noise=torch.from_numpy(inp["noise"]), weights=torch.from_numpy(inp["weights"]))
    torch.cuda.synchronize()
    e_mse = M.rel_err(res["mse"].cpu().numpy(), z["mse"])
    e_loss = abs(float(res["diffusion_loss"]) - c["loss"]) / abs(c["loss"])
    err = M.fixture_grad_err(_grads(m), c)
    worst = max(err, key=err.get)
    print(f"training_losses: mse rel {e_mse:.3e} (gate {float(z['tol_rel_mse']):.3e}); loss rel {e_loss:.3e} (gate {c['tol_rel_loss']:.3e}); "
          f"worst gradient {worst} rel {err[worst]:.3e} (gate {c['tol_rel']:.3e})")
    assert set(res) == {"mse", "loss", "diffusion_loss"} and float(res["loss"]) == float(res["diffusion_loss"])
    assert e_mse <= float(z["tol_rel_mse"]) and e_loss <= c["tol_rel_loss"]
    assert err[worst] <= c["tol_rel"], (worst, err[worst])
    ts.close()


def test_sgd_run_follows_the_reference_curve():
    """ten plain-SGD steps of the diffusion objective with the fixture's t and noise per step through loss_and_grads + torch.optim.SGD
    against the reference's float64 loss curve.  Gate: 4 x the reference's float32 curve's own deviation (not below the rounding of
    the one float32 each loss is returned as), printed.  Then the inference path sees the new weights."""
    import torch

    c, diffusion, batch = _objective("mdmtrain_sgd.npz")
    z, inp = c["z"], c["inputs"]
    c64, c32 = z["curve"], z["curve32"]
    gate = 4 * max(float(np.abs(c32 - c64).max()), 2.0 ** -24 * float(c64.max()))
    B, T = inp["x_start"].shape[0], inp["x_start"].shape[3]
    m, ts = _step(c["arch"], c["sd"], B, T)
    opt = torch.optim.SGD(m.parameters(), lr=float(z["lr"]))
    w = torch.from_numpy(inp["weights"])
    curve = []
    for k in range(len(c64)):
        opt.zero_grad()
        res = ts.loss_and_grads(diffusion, batch, t=torch.from_numpy(inp["t"][k]), noise=torch.from_numpy(inp["noise"][k]), weights=w)
        opt.step()
        curve.append(float(res["loss"].cpu()))
    dev = float(np.abs(np.array(curve) - c64).max())
    print(f"sgd curve {curve}; deviation {dev:.3e}; the reference's float32 deviation {float(np.abs(c32 - c64).max()):.3e}; gate {gate:.3e}")
    assert c64[-1] < c64[0] and dev <= gate
    m.refresh_hip_weights()
    x, t, b = _batch({**inp, "x_t": inp["x_start"], "t": inp["t"][0]})
    with torch.no_grad():
        a = ts.forward(x, t, b).cpu().numpy()
        ts.discard_forward()
        ref = m(x, t.to("cuda:0"), b).cpu().numpy()
    assert float(np.abs(a - ref).max() / np.abs(ref).max()) <= FIXTURE_TOL_OUT_MAX
    ts.close()


def test_zero_grad_between_steps_keeps_training():
    """optimizer.zero_grad() sets .grad to None by default: the next forward + backward has to write gradients the optimiser sees"""
    import torch

    arch = M.ARCH_L1_128
    sd, inp, _, G = _sweep_case(arch, 2, 7, False, 8000)
    m, ts = _step(arch, sd, 2, 7)
    opt = torch.optim.SGD(m.parameters(), lr=1e-2)
    (x, t, batch), g = _batch(inp), torch.from_numpy(G).to("cuda:0")
    ts.forward(x, t, batch).backward(g)
    first = {k: v.grad.clone() for k, v in m.named_parameters()}
    opt.zero_grad()
    assert all(v.grad is None for v in m.parameters())
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    ts.forward(x, t, batch).backward(g)
    for k, v in m.named_parameters():
        assert v.grad is not None and torch.equal(v.grad, first[k]), k
    opt.step()
    assert all(not torch.equal(v.detach(), before[k]) for k, v in m.named_parameters())
    for v in m.parameters():  # a gradient tensor assigned by the caller is bound where it is
        v.grad = torch.full_like(v, float("nan"))
    ts.forward(x, t, batch).backward(g)
    torch.cuda.synchronize()
    assert all(torch.isfinite(v.grad).all() for v in m.parameters())
    ts.close()


def test_refusals():
    """backward before forward, t out of range, the call limits, a second forward, an unbound tensor: the status, the message, nothing
    launched, and a following valid call works"""
    import torch

    from oakink2_tamf_amd.hip_backend import TamfError
    from oakink2_tamf_amd.model import interaction_segment_mdm_train as imt

    L = imt.lib()
    arch = M.ARCH_L1_128
    sd, inp, _, G = _sweep_case(arch, 2, 7, False, 7000)
    m, ts = _step(arch, sd, 2, 7)

    def untouched():  # nothing was launched: every gradient element is still the NaN it was filled with
        torch.cuda.synchronize()
        return all(bool(torch.isnan(v.grad).all()) for v in m.parameters())

    for v in m.parameters():
        v.grad.fill_(float("nan"))
    g = torch.zeros(2, 7, 99, device="cuda:0")
    rc = L.tamf_mdmtrain_backward(ts._h, ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(0))
    assert rc == -2 and "preceding tamf_mdmtrain_forward" in L.tamf_mdmtrain_last_error().decode()
    _, big, _, _ = _sweep_case(arch, 3, 7, False, 7001)
    with pytest.raises(TamfError, match="max_batch = 2"):
        ts.forward(*_batch(big))
    _, long_, _, _ = _sweep_case(arch, 2, 8, False, 7002)
    with pytest.raises(TamfError, match="max_frames = 7"):
        ts.forward(*_batch(long_))
    ts.dropout = 1.0
    with pytest.raises(TamfError, match="dropout_p"):
        ts.forward(*_batch(inp))
    ts.dropout = 0.0
    x, t, b = _batch(inp)
    with pytest.raises(ValueError, match=r"timesteps must be in \[0, 4999\]"):
        ts.forward(x, torch.tensor([3, 5000]), b)
    xt = x[:, :, 0, :].permute(0, 2, 1).contiguous()
    t_bad, t_ok = (ctypes.c_int32 * 2)(3, 5000), (ctypes.c_int32 * 2)(3, 4999)
    out = torch.empty(2, 7, 99, device="cuda:0")
    side = torch.zeros(2, dtype=torch.uint8, device="cuda:0")
    args = [ts._h, 2, 7, 2, None, ctypes.cast(t_bad, ctypes.c_void_p)] + [ctypes.c_void_p(v.data_ptr()) for v in (xt, b["text_embedding"], b["shape"], side,
            b["obj_embedding"], b["obj_traj"])] + [None, 0.0, 0, 0, ctypes.c_void_p(out.data_ptr()), None]
    assert L.tamf_mdmtrain_forward(*args) == -1 and "t[1] = 5000 outside [0, 4999]" in L.tamf_mdmtrain_last_error().decode()
    args[5] = ctypes.cast(t_ok, ctypes.c_void_p)
    args[3] = 4097
    assert L.tamf_mdmtrain_forward(*args) == -1 and "4096" in L.tamf_mdmtrain_last_error().decode()
    bad_num = (ctypes.c_int32 * 2)(1, 3)
    args[3], args[4] = 2, ctypes.cast(bad_num, ctypes.c_void_p)
    assert L.tamf_mdmtrain_forward(*args) == -1 and "obj_num[1] = 3" in L.tamf_mdmtrain_last_error().decode()
    assert L.tamf_mdmtrain_backward(ts._h, ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(0)) == -2  # (a refused forward is no forward)
    assert untouched()
    ref, tol, tol_out = _oracle_gates(sd, arch, inp, G, None)
    _check("after the refusals", _run(m, ts, inp, G), ref, tol, tol_out)
    with pytest.raises(RuntimeError, match="no backward yet"):
        ts.forward(x, t, b)
        ts.forward(x, t, b)
    ts.discard_forward()
    ts.close()

    m2 = _model(arch, sd)
    ts2 = imt.InterationSegmentMDMTrainStep.__new__(imt.InterationSegmentMDMTrainStep)
    bind = imt.InterationSegmentMDMTrainStep.bind
    imt.InterationSegmentMDMTrainStep.bind = lambda self, skip=(): bind(self, skip=("embed_text.bias",))
    try:
        ts2.__init__(m2, 2, 7)
    finally:
        imt.InterationSegmentMDMTrainStep.bind = bind
    for v in m2.parameters():
        v.grad.fill_(float("nan"))
    with pytest.raises(TamfError, match="error -4: missing binding 'embed_text.bias'"):
        ts2.forward(x, t, b)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v.grad).all()) for v in m2.parameters())
    ts2.bind()
    _check("after the missing binding", _run(m2, ts2, inp, G), ref, tol, tol_out)
    ts2.close()
