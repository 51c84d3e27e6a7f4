"""The refiner's training step (libtamf_refinetrain.so, SegmentRefineTrainStep) on the MI355X: the reference's output and gradients
(tests/golden/refinetrain_*.npz) inside the gates measured on the reference itself, float64 autograd through
oracle.mdm_oracle.refine_forward over a shape sweep, non-finite inputs, dropout with the library's own masks injected into the float64
restatement, determinism and batch invariance bit for bit, the inference path on the same weights, a short SGD run against the
oracle's loss curve, and the refusals.

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
import refine_train_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")
FIXTURES = ("refinetrain_tiny.npz", "refinetrain_l1_ff16.npz", "refinetrain_deep.npz")
_TOLS = [np.load(os.path.join(GOLDEN, f)) for f in FIXTURES + ("refinetrain_e2e.npz",)]
FIXTURE_TOL_MAX, FIXTURE_TOL_OUT_MAX = max(float(z["tol_rel"]) for z in _TOLS), max(float(z["tol_rel_out"]) for z in _TOLS)
ARCHS = {"l1_ff16": R.ARCH_L1, "tiny": R.ARCH_TINY}


def _model(arch, sd, p=0.0):
    import torch

    from oakink2_tamf_amd.model.segment_refine_model import SegmentRefineModel

    m = SegmentRefineModel(**R.arch_dict(arch), dropout=p, precision="f32").to("cuda:0")
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    return m


def _batch(inp, rows=None):
    import torch

    sl = slice(None) if rows is None else rows
    b = {k: torch.from_numpy(np.ascontiguousarray(inp[k][sl])).to("cuda:0") for k in ("sample_pose_repr", "h2o_dist", "shape", "obj_embedding", "obj_traj")}
    b["hand_side"] = [inp["hand_side"][i] for i in (range(len(inp["hand_side"])) if rows is None else rows)]
    return b


def _step(arch, sd, B, T, p=0.0, seed=0):
    from oakink2_tamf_amd.model.segment_refine_train import SegmentRefineTrainStep

    m = _model(arch, sd, p)
    return m, SegmentRefineTrainStep(m, B, T, dropout=p, seed=seed)


def _run(m, ts, inp, G, obj_num=None, clip_ids=None, step=0, rows=None):
    """one forward + backward of loss = sum(G * out), every gradient buffer pre-filled with NaN -> (out, {key: gradient}) as numpy"""
    import torch

    for p_ in m.parameters():
        p_.grad.fill_(float("nan"))
    out = ts.forward(_batch(inp, rows), obj_num=obj_num, clip_ids=clip_ids, step=step)
    g = torch.from_numpy(np.ascontiguousarray(np.asarray(G, np.float32)[slice(None) if rows is None else rows])).to("cuda:0")
    (out * g).sum().backward()
    torch.cuda.synchronize()
    return out.detach().cpu().numpy().copy(), {k: v.grad.cpu().numpy().copy() for k, v in m.named_parameters()}


def _masks(ts, arch, B, T, step=0, clip_ids=None):
    import torch

    return {s: torch.stack([ts.dropout_mask(step, b if clip_ids is None else clip_ids[b], s, r, c) for b in range(B)]).cpu()
            for s, (r, c) in R.site_shapes(arch, T).items()}


def _check(tag, got, ref, tol, tol_out):
    out, grads = got
    assert set(grads) == set(ref[2]) and not set(grads) & set(R.BUFFERS)
    err = R.grad_rel_err(grads, ref[2])
    worst = max(err, key=err.get)
    e_out = R.rel_err(out, ref[0])
    print(f"{tag}: output rel {e_out:.3e} (gate {tol_out:.3e}); worst gradient {worst} rel {err[worst]:.3e} (gate {tol:.3e})")
    assert e_out <= tol_out, (tag, e_out, tol_out)
    assert err[worst] <= tol, (tag, worst, err[worst], tol)


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixture(name):
    """output and every gradient of the reference's own module inside 4 x the reference's float32 error; every gradient element
    written (the buffers start as NaN).  Measured on the MI355X: see the table in DESIGN.md section 4."""
    c = R.load_case(os.path.join(GOLDEN, name))
    B, T = c["inputs"]["sample_pose_repr"].shape[:2]
    m, ts = _step(c["arch"], c["sd"], B, T)
    out, grads = _run(m, ts, c["inputs"], c["G"], c["obj_num"])
    assert not any(np.isnan(g).any() for g in grads.values())
    err = R.fixture_grad_err(grads, c)
    worst = max(err, key=err.get)
    e_out = R.rel_err(out, c["out"])
    loss = float((c["G"].astype(np.float64) * out.astype(np.float64)).sum())
    print(f"{name}: output rel {e_out:.3e} (gate {c['tol_rel_out']:.3e}); worst gradient {worst} rel {err[worst]:.3e} (gate {c['tol_rel']:.3e}); "
          f"loss rel {abs(loss - c['loss']) / abs(c['loss']):.3e}")
    assert e_out <= c["tol_rel_out"]
    assert err[worst] <= c["tol_rel"], (worst, err[worst])
    ts.close()


def _sweep_case(arch, B, T, ragged, seed):
    sd = R.seeded_state_dict(arch, seed)
    inp, obj_num = R.seeded_inputs(arch, B, T, 2, seed + 1, ragged)
    G = np.random.default_rng(seed + 2).normal(size=(B, T, arch.input_dim)).astype(np.float32)
    return sd, inp, obj_num, G


def _oracle_gates(sd, arch, inp, G, obj_num):
    """float64 autograd through the oracle, and the gates 4 x (the oracle's float32 autograd against it), capped at the fixtures'"""
    import torch

    ref = R.loss_and_grads(sd, arch, inp, G, obj_num, forward=R.oracle_forward)
    r32 = R.loss_and_grads(sd, arch, inp, G, obj_num, dtype=torch.float32, forward=R.oracle_forward)
    m_g, m_o = 4 * max(R.grad_rel_err(r32[2], ref[2]).values()), 4 * R.rel_err(r32[0], ref[0])
    print(f"gates measured at test time: gradients {m_g:.3e} (largest fixture gate {FIXTURE_TOL_MAX:.3e}), output {m_o:.3e} ({FIXTURE_TOL_OUT_MAX:.3e})")
    return ref, min(m_g, FIXTURE_TOL_MAX), min(m_o, FIXTURE_TOL_OUT_MAX)


@pytest.mark.parametrize("ragged", [False, True], ids=["padded", "ragged"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 13, 14, 61, 62, 196])  # S = 4, 16, 17, 64, 65, 199: below, at and across the 16-row and 64-row tiles
@pytest.mark.parametrize("arch_name", sorted(ARCHS))
def test_sweep_against_oracle_autograd(arch_name, T, B, ragged):
    arch = ARCHS[arch_name]
    sd, inp, obj_num, G = _sweep_case(arch, B, T, ragged, 1000 + 7 * T + B)
    ref, tol, tol_out = _oracle_gates(sd, arch, inp, G, obj_num)
    m, ts = _step(arch, sd, B, T)
    _check(f"{arch_name} T{T} B{B} {'ragged' if ragged else 'padded'}", _run(m, ts, inp, G, obj_num), ref, tol, tol_out)
    ts.close()


def test_arch_refine_against_oracle_autograd():
    """config/arch_refine.yml itself (latent 256, 4 heads, ff 1024, 8 layers, 768-wide object embeddings) at B 2, T 14"""
    import yaml

    with open(os.path.join(HERE, "..", "config", "arch_refine.yml")) as f:
        cfg = yaml.safe_load(f)["model"]
    arch = R.mo.Arch(kind="R", **{k: int(cfg[k]) for k in R.ARCH_NAMES if k in cfg})
    assert (arch.latent_dim, arch.num_heads, arch.ff_size, arch.num_layers) == (256, 4, 1024, 8)
    sd, inp, obj_num, G = _sweep_case(arch, 2, 14, True, 3000)
    ref, tol, tol_out = _oracle_gates(sd, arch, inp, G, obj_num)
    m, ts = _step(arch, sd, 2, 14)
    _check("arch_refine T14 B2", _run(m, ts, inp, G, obj_num), ref, tol, tol_out)
    ts.close()


def test_nonfinite_inputs():
    """NaN in one clip's obj_embedding and inf in its h2o_dist: the three nan_to_num pass gradient where their input is finite - the
    gradients equal the float64 autograd's where those are finite and are NaN where they are NaN (0 * NaN in the weight gradients
    behind the mask)"""
    arch = R.ARCH_TINY
    sd, inp, obj_num, G = _sweep_case(arch, 3, 14, False, 4000)
    inp["obj_embedding"][1, 0, 3] = np.nan
    inp["h2o_dist"][1, 2, 5] = np.inf
    ref, tol, tol_out = _oracle_gates(sd, arch, inp, G, obj_num)
    assert any(np.isnan(g).any() for g in ref[2].values()) and not all(np.isnan(g).all() for g in ref[2].values())
    m, ts = _step(arch, sd, 3, 14)
    _check("nonfinite", _run(m, ts, inp, G, obj_num), ref, tol, tol_out)
    ts.close()


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name", ["refinetrain_tiny.npz", "refinetrain_l1_ff16.npz"])
def test_dropout_with_the_librarys_masks(name, p):
    """the library's own keep-masks (dropout_mask) injected into the float64 restatement; the fixture's gates"""
    c = R.load_case(os.path.join(GOLDEN, name))
    B, T = c["inputs"]["sample_pose_repr"].shape[:2]
    m, ts = _step(c["arch"], c["sd"], B, T, p=p, seed=77)
    clip_ids = [5 + 3 * b for b in range(B)]
    got = _run(m, ts, c["inputs"], c["G"], c["obj_num"], clip_ids=clip_ids, step=4)
    masks = _masks(ts, c["arch"], B, T, step=4, clip_ids=clip_ids)
    kept = np.mean([float(v.float().mean()) for v in masks.values()])
    assert abs(kept - (1 - p)) < 0.05
    ref = R.loss_and_grads(c["sd"], c["arch"], c["inputs"], c["G"], c["obj_num"], masks, p)
    _check(f"{name} p={p}", got, ref, c["tol_rel"], c["tol_rel_out"])
    ts.close()


def test_tiny_p_gives_the_bits_of_no_dropout():
    """p = 2^-32: the threshold is 1, every draw keeps (none of these draws is 0) and the scale rounds to 1 - the bits of p = 0"""
    c = R.load_case(os.path.join(GOLDEN, "refinetrain_tiny.npz"))
    B, T = c["inputs"]["sample_pose_repr"].shape[:2]
    m0, ts0 = _step(c["arch"], c["sd"], B, T, p=0.0)
    m1, ts1 = _step(c["arch"], c["sd"], B, T, p=2.0 ** -32)
    a, b = _run(m0, ts0, c["inputs"], c["G"], c["obj_num"]), _run(m1, ts1, c["inputs"], c["G"], c["obj_num"])
    assert all(bool(v.all()) for v in _masks(ts1, c["arch"], B, T).values())
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])
    ts0.close()
    ts1.close()


def test_clip_invariance_and_determinism():
    """with obj_num given, a clip's forward has the same bits alone and at another batch position under the same clip id, and other
    bits under another id; the same forward + backward twice gives identical bits in every gradient, overwritten, not accumulated"""
    import torch

    arch = R.ARCH_TINY
    sd, inp, obj_num, G = _sweep_case(arch, 3, 14, True, 5000)
    m, ts = _step(arch, sd, 3, 14, p=0.3, seed=11)
    ids = [40, 41, 42]
    full, g1 = _run(m, ts, inp, G, obj_num, clip_ids=ids, step=2)
    full2, g2 = _run(m, ts, inp, G, obj_num, clip_ids=ids, step=2)  # (the gradient buffers were NaN again before this call)
    assert np.array_equal(full, full2) and all(np.array_equal(g1[k], g2[k]) for k in g1)
    assert not any(np.isnan(g).any() for g in g2.values())
    with torch.no_grad():
        alone = ts.forward(_batch(inp, [1]), obj_num=[obj_num[1]], clip_ids=[41], step=2).cpu().numpy()
        ts.discard_forward()
        moved = ts.forward(_batch(inp, [2, 1]), obj_num=[obj_num[2], obj_num[1]], clip_ids=[42, 41], step=2).cpu().numpy()
        ts.discard_forward()
        other = ts.forward(_batch(inp, [1]), obj_num=[obj_num[1]], clip_ids=[43], step=2).cpu().numpy()
        ts.discard_forward()
    assert np.array_equal(alone[0], full[1]) and np.array_equal(moved[1], full[1]) and np.array_equal(moved[0], full[2])
    assert not np.array_equal(other[0], full[1])
    ts.close()


def test_forward_agrees_with_the_inference_path():
    """p = 0: the training forward against SegmentRefineModel(precision="f32") on the same weights, inside the fixture's output gate"""
    import torch

    c = R.load_case(os.path.join(GOLDEN, "refinetrain_tiny.npz"))
    B, T = c["inputs"]["sample_pose_repr"].shape[:2]
    m, ts = _step(c["arch"], c["sd"], B, T)
    batch = _batch(c["inputs"])
    with torch.no_grad():
        a = ts.forward(batch).cpu().numpy()  # (padded object means: the reference's forward on the batch it is given)
        ts.discard_forward()
        b = m(batch)["refine_pose_repr"].cpu().numpy()
    e = float(np.abs(a - b).max() / np.abs(b).max())
    print(f"training forward against the inference path: rel {e:.3e} (gate {c['tol_rel_out']:.3e})")
    assert e <= c["tol_rel_out"]
    ts.close()


def _sgd_curve_oracle(sd_np, arch, inp, target, dtype, steps, lr):
    import torch

    sd = R.leaf_state_dict(sd_np, dtype)
    params = [v for k, v in sd.items() if k not in R.BUFFERS]
    opt = torch.optim.SGD(params, lr=lr)
    x, h, t = (torch.from_numpy(a).to(dtype) for a in (inp["sample_pose_repr"], inp["h2o_dist"], target))
    curve = []
    for _ in range(steps):
        opt.zero_grad()
        loss = ((R.mo.refine_forward(sd, arch, x, h, R.cond_of(inp, dtype), dtype) - t) ** 2).mean()
        loss.backward()
        opt.step()
        curve.append(float(loss.detach()))
    return np.array(curve)


def test_sgd_run_follows_the_oracle_curve():
    """ten plain-SGD steps (lr 1e-2) on the tiny architecture with an MSE-to-pose_repr loss through SegmentRefineTrainStep.forward +
    torch.optim.SGD against the float64 oracle's loss curve.  Gate: 4 x the float32 oracle curve's own deviation (not below the
    rounding of the one float32 each loss is returned as), measured here and printed.  Then the inference path sees the new weights."""
    import torch

    arch, steps, lr = R.ARCH_TINY, 10, 1e-2
    sd, inp, _, _ = _sweep_case(arch, 3, 14, False, 6000)
    target = (inp["sample_pose_repr"] + 0.1 * np.random.default_rng(6001).normal(size=inp["sample_pose_repr"].shape)).astype(np.float32)
    c64 = _sgd_curve_oracle(sd, arch, inp, target, torch.float64, steps, lr)
    c32 = _sgd_curve_oracle(sd, arch, inp, target, torch.float32, steps, lr)
    gate = 4 * max(float(np.abs(c32 - c64).max()), 2.0 ** -24 * float(c64.max()))
    m, ts = _step(arch, sd, 3, 14)
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    batch, tgt = _batch(inp), torch.from_numpy(target).to("cuda:0")
    curve = []
    for _ in range(steps):
        opt.zero_grad()
        loss = ((ts.forward(batch) - tgt) ** 2).mean()
        loss.backward()
        opt.step()
        curve.append(float(loss.detach().cpu()))
    dev = float(np.abs(np.array(curve) - c64).max())
    print(f"sgd curve {curve}; deviation {dev:.3e}; float32 oracle's deviation {float(np.abs(c32 - c64).max()):.3e}; gate {gate:.3e}")
    assert c64[-1] < c64[0] and dev <= gate
    m.refresh_hip_weights()
    with torch.no_grad():
        a = ts.forward(batch).cpu().numpy()
        ts.discard_forward()
        b = m(batch)["refine_pose_repr"].cpu().numpy()
    assert float(np.abs(a - b).max() / np.abs(b).max()) <= FIXTURE_TOL_OUT_MAX
    ts.close()


def test_zero_grad_between_steps_keeps_training():
    """optimizer.zero_grad() sets .grad to None by default: the next forward + backward has to write gradients the optimiser sees"""
    import torch

    arch = R.ARCH_L1
    sd, inp, _, G = _sweep_case(arch, 2, 7, False, 8000)
    m, ts = _step(arch, sd, 2, 7)
    opt = torch.optim.SGD(m.parameters(), lr=1e-2)
    batch, g = _batch(inp), torch.from_numpy(G).to("cuda:0")
    ts.forward(batch).backward(g)
    first = {k: v.grad.clone() for k, v in m.named_parameters()}
    opt.zero_grad()
    assert all(v.grad is None for v in m.parameters())
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    ts.forward(batch).backward(g)
    for k, v in m.named_parameters():
        assert v.grad is not None and torch.equal(v.grad, first[k]), k
    opt.step()
    assert all(not torch.equal(v.detach(), before[k]) for k, v in m.named_parameters())
    for v in m.parameters():  # a gradient tensor assigned by the caller is bound where it is
        v.grad = torch.full_like(v, float("nan"))
    ts.forward(batch).backward(g)
    torch.cuda.synchronize()
    assert all(torch.isfinite(v.grad).all() for v in m.parameters())
    ts.close()


def test_refusals():
    """each limit, backward before forward, an unbound tensor: the status, the message, nothing launched, and a following valid call works"""
    import torch

    from oakink2_tamf_amd.hip_backend import TamfError, _Arch
    from oakink2_tamf_amd.model import segment_refine_train as srt

    L = srt.lib()
    good = dict(input_dim=99, obj_input_dim=9, hand_shape_dim=10, obj_embed_dim=32, latent_dim=64, ff_size=16, num_layers=1, num_heads=1, h2o_dim=778)

    def create(arch, max_batch=2, max_frames=7):
        a = _Arch(arch["input_dim"], arch["obj_input_dim"], arch["hand_shape_dim"], arch["obj_embed_dim"], arch["latent_dim"], arch["ff_size"],
                  arch["num_layers"], arch["num_heads"], 0, arch["h2o_dim"], 1)
        h = ctypes.c_void_p()
        rc = L.tamf_refinetrain_create(ctypes.byref(a), max_batch, max_frames, 0, ctypes.byref(h))
        msg = L.tamf_refinetrain_last_error().decode()
        if rc == 0:
            L.tamf_refinetrain_destroy(h)
        return rc, msg

    bad = [(dict(good, num_heads=9, latent_dim=576), "num_heads"), (dict(good, num_heads=0), "num_heads"), (dict(good, latent_dim=128), "latent_dim = 64 \\* num_heads"),
           (dict(good, ff_size=24), "ff_size"), (dict(good, ff_size=4112), "4096"), (dict(good, num_layers=0), "num_layers"), (dict(good, num_layers=65), "64")]
    bad += [(dict(good, **{k: v}), k) for k in ("input_dim", "obj_input_dim", "hand_shape_dim", "obj_embed_dim", "h2o_dim") for v in (0, 4097)]
    import re
    for arch, word in bad:
        rc, msg = create(arch)
        assert rc == -1 and re.search(word, msg), (arch, rc, msg)
    for kw, word in ((dict(max_frames=1022), "1021"), (dict(max_frames=0), "max_frames"), (dict(max_batch=0), "max_batch"), (dict(max_batch=65536), "65535")):
        rc, msg = create(good, **kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert create(good)[0] == 0 and create(dict(good, num_heads=8, latent_dim=512, ff_size=4096), 1, 1021)[0] == 0

    arch = R.ARCH_L1
    sd, inp, _, G = _sweep_case(arch, 2, 7, False, 7000)
    m, ts = _step(arch, sd, 2, 7)

    def nan_grads():
        for v in m.parameters():
            v.grad.fill_(float("nan"))

    def untouched():  # nothing was launched: every gradient element is still the NaN it was filled with
        torch.cuda.synchronize()
        return all(bool(torch.isnan(v.grad).all()) for v in m.parameters())

    nan_grads()
    g = torch.zeros(2, 7, 99, device="cuda:0")
    rc = L.tamf_refinetrain_backward(ts._h, ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(0))
    assert rc == -2 and "preceding tamf_refinetrain_forward" in L.tamf_refinetrain_last_error().decode()
    _, big, _, _ = _sweep_case(arch, 3, 7, False, 7001)
    with pytest.raises(TamfError, match="max_batch = 2"):
        ts.forward(_batch(big))
    _, long_, _, _ = _sweep_case(arch, 2, 8, False, 7002)
    with pytest.raises(TamfError, match="max_frames = 7"):
        ts.forward(_batch(long_))
    ts.dropout = 1.0
    with pytest.raises(TamfError, match="dropout_p"):
        ts.forward(_batch(inp))
    ts.dropout = 0.0
    x = _batch(inp)
    args = [ts._h, 2, 7, 4097, None] + [ctypes.c_void_p(x[k].data_ptr()) for k in ("sample_pose_repr", "h2o_dist", "shape")] + \
        [ctypes.c_void_p(x["shape"].data_ptr()), ctypes.c_void_p(x["obj_embedding"].data_ptr()), ctypes.c_void_p(x["obj_traj"].data_ptr()), None,
         0.0, 0, 0, ctypes.c_void_p(x["sample_pose_repr"].data_ptr()), None]
    assert L.tamf_refinetrain_forward(*args) == -1 and "4096" in L.tamf_refinetrain_last_error().decode()
    bad_num = (ctypes.c_int32 * 2)(1, 3)
    args[3], args[4] = 2, ctypes.cast(bad_num, ctypes.c_void_p)
    assert L.tamf_refinetrain_forward(*args) == -1 and "obj_num[1] = 3" in L.tamf_refinetrain_last_error().decode()
    assert L.tamf_refinetrain_backward(ts._h, ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(0)) == -2  # (a refused forward is no forward)
    assert untouched()
    ref, tol, tol_out = _oracle_gates(sd, arch, inp, G, None)
    _check("after the refusals", _run(m, ts, inp, G), ref, tol, tol_out)
    with pytest.raises(RuntimeError, match="no backward yet"):
        ts.forward(_batch(inp))
        ts.forward(_batch(inp))
    ts.discard_forward()
    ts.close()

    m2 = _model(arch, sd)
    ts2 = srt.SegmentRefineTrainStep.__new__(srt.SegmentRefineTrainStep)
    bind = srt.SegmentRefineTrainStep.bind
    srt.SegmentRefineTrainStep.bind = lambda self, skip=(): bind(self, skip=("input_merge.2.bias",))
    try:
        ts2.__init__(m2, 2, 7)
    finally:
        srt.SegmentRefineTrainStep.bind = bind
    for v in m2.parameters():
        v.grad.fill_(float("nan"))
    with pytest.raises(TamfError, match="error -4: missing binding 'input_merge.2.bias'"):
        ts2.forward(_batch(inp))
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v.grad).all()) for v in m2.parameters())
    ts2.bind()
    m, ts = m2, ts2
    _check("after the missing binding", _run(m2, ts2, inp, G), ref, tol, tol_out)
    ts2.close()
