"""GPU: the backward of the native MANO layer (tamf_mano_backward, HipManoLayer(differentiable=True)) against float64 autograd through
the restatement of the definition (tests/mano_restatement.py) on synthetic MANO-shaped arrays (tests/mano_fixture.py).

Tolerance: measured, not chosen - the rule of test_mano_gpu.py.  Per case and per tensor e32 = max |g32 - g64| / max |g64| of the
float32 restatement's autograd against the float64 one on the case's own inputs and upstream, and the gate on the HIP gradient is
4 * e32: both sides are fp32 sums of the same terms in different orders; the factor covers the ordering and nothing more."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import mano_fixture as F  # noqa: E402
import mano_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAMF_ERR_INVALID = -1
_REF = {}


def _arrays(V, seed=0):
    from oakink2_tamf_amd.mano import ManoArrays

    key = ("arrays", V, seed)
    if key not in _REF:
        _REF[key] = ManoArrays(**F.synthetic_arrays(V, seed))
    return _REF[key]


def _layer(V, center, differentiable=False):
    from oakink2_tamf_amd.mano import HipManoLayer

    key = ("layer", V, center, differentiable)
    if key not in _REF:
        _REF[key] = HipManoLayer(_arrays(V), center_idx=center, device=DEV, differentiable=differentiable)
    return _REF[key]


def _inputs(N, seed=0, scale=None):
    q, b = F.random_inputs(N, seed, scale)
    return torch.from_numpy(q).float(), torch.from_numpy(b).float()


def _upstream(V, N, seed):
    g = torch.Generator().manual_seed(1234 + seed)
    return torch.randn(N, V, 3, generator=g), torch.randn(N, 21, 3, generator=g)


def _restatement_grads(V, center, q32, b32, gv, gj, dtype):
    """autograd through the restatement in `dtype` of (v * gv).sum() + (j * gj).sum(); gv / gj None = that output unused"""
    m = R.to_torch(_arrays(V), dtype)
    q, b = q32.to(dtype).requires_grad_(True), b32.to(dtype).requires_grad_(True)
    v, j, _ = R.mano_forward(m, q, b, center)
    loss = 0
    if gv is not None:
        loss = loss + (v * gv.to(dtype)).sum()
    if gj is not None:
        loss = loss + (j * gj.to(dtype)).sum()
    dq, db = torch.autograd.grad(loss, [q, b])
    return dq.double(), db.double()


def _reference(V, N, center, kind, which):
    """(q, b, gv, gj, dq64, db64, e32 of dquat, e32 of dbetas); computed once per case and left unchanged"""
    key = ("ref", V, N, center, kind, which)
    if key not in _REF:
        scale = np.where(np.arange(16) % 2 == 0, 0.5, 3.0) if kind == "nonunit" else None
        q, b = _inputs(N, seed=N, scale=scale)
        gv, gj = _upstream(V, N, N)
        if which == "verts":
            gj = None
        if which == "joints":
            gv = None
        dq64, db64 = _restatement_grads(V, center, q, b, gv, gj, torch.float64)
        dq32, db32 = _restatement_grads(V, center, q, b, gv, gj, torch.float32)
        eq = float((dq32 - dq64).abs().max() / dq64.abs().max())
        eb = float((db32 - db64).abs().max() / db64.abs().max())
        _REF[key] = (q, b, gv, gj, dq64, db64, eq, eb)
    return _REF[key]


def _dev(t):
    return None if t is None else t.to(DEV)


CASES = [(778, N, c, None, "both") for N in (1, 15, 16, 17, 33) for c in (0, None)]
CASES += [(20, 17, 0, None, "both"), (20, 17, None, None, "both"), (778, 17, 8, None, "both"), (778, 17, 0, "nonunit", "both")]
CASES += [(778, 17, 0, None, "verts"), (778, 17, 0, None, "joints"), (778, 17, 0, None, "nodbetas")]


@pytest.mark.parametrize("V,N,center,kind,which", CASES,
                         ids=[f"V{V}-N{N}-c{c}{'-' + k if k else ''}{'-' + w if w != 'both' else ''}" for V, N, c, k, w in CASES])
def test_gradient_parity_with_float64_autograd(V, N, center, kind, which):
    q, b, gv, gj, dq64, db64, eq32, eb32 = _reference(V, N, center, kind, "both" if which == "nodbetas" else which)
    layer = _layer(V, center)
    dq, db = layer.backward_raw(q.to(DEV), b.to(DEV), _dev(gv), _dev(gj), want_dbetas=which != "nodbetas")
    assert dq.shape == (N, 16, 4) and dq.dtype == torch.float32 and dq.is_cuda
    eq = float((dq.cpu().double() - dq64).abs().max() / dq64.abs().max())
    eb = float("nan") if db is None else float((db.cpu().double() - db64).abs().max() / db64.abs().max())
    print(f"MANO-GRAD V={V} N={N} center={center} {kind or 'unit'} {which}: dquat e32 {eq32:.3e} hip {eq:.3e} gate {4 * eq32:.3e} | "
          f"dbetas e32 {eb32:.3e} hip {eb:.3e} gate {4 * eb32:.3e}")
    assert eq32 > 0 and eb32 > 0
    assert np.isfinite(eq) and eq <= 4 * eq32
    if which == "nodbetas":
        assert db is None
        full = layer.backward_raw(q.to(DEV), b.to(DEV), _dev(gv), _dev(gj))[0]
        assert torch.equal(full, dq)  # dbetas_out NULL: the same dquat, bit for bit
    else:
        assert db.shape == (N, 10) and np.isfinite(eb) and eb <= 4 * eb32


def test_bits_do_not_depend_on_the_batch_the_position_or_the_launch():
    """a frame alone = at positions 0, 15, 16, 32 of a batch of 33 = after set_tiles(1 | 2 | 4) = in a second identical call;
    outputs pre-filled with NaN are fully overwritten"""
    from oakink2_tamf_amd.hip_backend import _stream_ptr
    from oakink2_tamf_amd.mano import _bind

    layer = _layer(778, 0)
    q, b = _inputs(33, seed=5)
    gv, gj = _upstream(778, 33, 5)
    q, b, gv, gj = q.to(DEV), b.to(DEV), gv.to(DEV), gj.to(DEV)
    full_q, full_b = layer.backward_raw(q, b, gv, gj)
    again_q, again_b = layer.backward_raw(q, b, gv, gj)
    assert torch.equal(full_q, again_q) and torch.equal(full_b, again_b)
    assert torch.isfinite(full_q).all() and torch.isfinite(full_b).all() and float(full_q.abs().max()) > 0
    for k in (0, 15, 16, 32):
        one_q, one_b = layer.backward_raw(q[k: k + 1], b[k: k + 1], gv[k: k + 1], gj[k: k + 1])
        assert torch.equal(one_q[0], full_q[k]) and torch.equal(one_b[0], full_b[k]), k
    # frame 7 moved to the positions 0, 15, 16, 32 of the batch
    for pos in (0, 15, 16, 32):
        perm = list(range(33))
        perm[pos], perm[7] = perm[7], perm[pos]
        perm = torch.tensor(perm, device=DEV)
        pq, pb = layer.backward_raw(q[perm], b[perm], gv[perm], gj[perm])
        assert torch.equal(pq[pos], full_q[7]) and torch.equal(pb[pos], full_b[7]), pos
        assert torch.equal(pq, full_q[perm]) and torch.equal(pb, full_b[perm])
    try:
        for tiles in (1, 2, 4):
            layer.set_tiles(tiles)
            tq, tb = layer.backward_raw(q, b, gv, gj)
            assert torch.equal(tq, full_q) and torch.equal(tb, full_b), tiles
    finally:
        layer.set_tiles(0)
    # the C call on NaN-filled outputs
    lib = _bind()
    dq = torch.full((33, 16, 4), float("nan"), device=DEV)
    db = torch.full((33, 10), float("nan"), device=DEV)
    rc = lib.tamf_mano_backward(layer._model, q.data_ptr(), b.data_ptr(), 33, gv.data_ptr(), gj.data_ptr(), dq.data_ptr(), db.data_ptr(),
                                _stream_ptr(torch.device(DEV)))
    assert rc == 0
    assert torch.equal(dq, full_q) and torch.equal(db, full_b)


def test_autograd_binding():
    from oakink2_tamf_amd.mano import HipManoLayer

    V, N = 778, 17
    plain, diff = _layer(V, 0), _layer(V, 0, differentiable=True)
    q0, b0 = _inputs(N, seed=9)
    gv, gj = _upstream(V, N, 9)
    gv, gj = gv.to(DEV), gj.to(DEV)
    q, b = q0.to(DEV).requires_grad_(True), b0.to(DEV).requires_grad_(True)
    out = diff(pose_coeffs=q, betas=b)
    ref = plain(pose_coeffs=q.detach(), betas=b.detach())
    assert torch.equal(out.verts, ref.verts) and torch.equal(out.joints, ref.joints)  # the inference layer's bits
    loss = (out.verts * gv).sum() + (out.joints * gj).sum()
    loss.backward()
    want_q, want_b = plain.backward_raw(q.detach(), b.detach(), gv, gj)
    assert torch.equal(q.grad, want_q) and torch.equal(b.grad, want_b)
    # an output nothing depends on reaches the kernel as NULL: the same bits as the direct call with NULL
    for use in ("verts", "joints"):
        q.grad = b.grad = None
        out = diff(pose_coeffs=q, betas=b)
        ((out.verts * gv).sum() if use == "verts" else (out.joints * gj).sum()).backward()
        want_q, want_b = plain.backward_raw(q.detach(), b.detach(), gv if use == "verts" else None, gj if use == "joints" else None)
        assert torch.equal(q.grad, want_q) and torch.equal(b.grad, want_b), use
    # zero upstream: exactly zero gradients
    q.grad = b.grad = None
    out = diff(pose_coeffs=q, betas=b)
    ((out.verts * 0).sum() + (out.joints * 0).sum()).backward()
    assert float(q.grad.abs().max()) == 0.0 and float(b.grad.abs().max()) == 0.0
    # with_joints=False; betas without grad
    q.grad = None
    bn = b0.to(DEV)
    only = diff.forward(q, bn, with_joints=False)
    assert only.joints is None and torch.equal(only.verts, ref.verts)
    (only.verts * gv).sum().backward()
    assert bn.grad is None and torch.equal(q.grad, plain.backward_raw(q.detach(), bn, gv, None, want_dbetas=False)[0])
    # no grad needed: the inference path, no graph
    assert diff(pose_coeffs=q.detach(), betas=bn).verts.grad_fn is None
    # double backward is refused
    q.grad = None
    out = diff(pose_coeffs=q, betas=b)
    with pytest.raises(RuntimeError, match="double backward is not supported"):
        torch.autograd.grad((out.verts * gv).sum(), [q], create_graph=True)
    # N = 0: empty gradients, nothing launched
    qe, be = torch.zeros(0, 16, 4, device=DEV, requires_grad=True), torch.zeros(0, 10, device=DEV, requires_grad=True)
    oe = diff(pose_coeffs=qe, betas=be)
    (oe.verts.sum() + oe.joints.sum()).backward()
    assert qe.grad.shape == (0, 16, 4) and be.grad.shape == (0, 10)
    # the default layer still refuses
    with pytest.raises(RuntimeError, match="inference only"):
        plain(pose_coeffs=q, betas=bn)
    small = HipManoLayer(_arrays(20), center_idx=None, device=DEV, differentiable=True)
    qs = _inputs(3)[0].to(DEV).requires_grad_(True)
    small(pose_coeffs=qs, betas=_inputs(3)[1].to(DEV)).joints.sum().backward()
    assert torch.isfinite(qs.grad).all() and float(qs.grad.abs().max()) > 0
    small.close()


def _fit_curve(step_fn, q0, b0, steps, lr):
    """`steps` SGD steps on (quat, betas) from (q0, b0); step_fn(q, b) -> (loss, dq, db)"""
    q, b, curve = q0.clone(), b0.clone(), []
    for _ in range(steps):
        loss, dq, db = step_fn(q, b)
        curve.append(float(loss.detach()))
        q, b = q - lr * dq, b - lr * db
    return np.array(curve)


def test_ten_step_fit_follows_the_float64_curve():
    """ten SGD steps fitting 17 frames' quaternions and betas to target joints from a fixed start: the loss curve against the float64
    restatement's; the deviation within 4 x that of the float32 restatement's curve (the shape of test_enctrain_gpu's sgd test)"""
    V, N, steps, lr = 778, 17, 10, 50.0
    a = _arrays(V)
    qt, bt = _inputs(N, seed=21)
    q0, b0 = _inputs(N, seed=22)
    q0 = torch.nn.functional.normalize(0.7 * qt + 0.3 * q0, dim=-1)  # a start near enough for SGD to make progress in ten steps
    b0 = 0.5 * bt
    target = R.mano_forward(R.to_torch(a, torch.float64), qt.double(), bt.double(), 0)[1]

    def restatement(dtype):
        m, tgt = R.to_torch(a, dtype), target.to(dtype)

        def step(q, b):
            q, b = q.detach().requires_grad_(True), b.detach().requires_grad_(True)
            loss = ((R.mano_forward(m, q, b, 0)[1] - tgt) ** 2).sum(-1).mean()
            dq, db = torch.autograd.grad(loss, [q, b])
            return loss, dq, db

        return step

    c64 = _fit_curve(restatement(torch.float64), q0.double(), b0.double(), steps, lr)
    c32 = _fit_curve(restatement(torch.float32), q0, b0, steps, lr)
    layer, tgt = _layer(V, 0, differentiable=True), target.float().to(DEV)

    def hip(q, b):
        q, b = q.detach().requires_grad_(True), b.detach().requires_grad_(True)
        loss = ((layer(pose_coeffs=q, betas=b).joints - tgt) ** 2).sum(-1).mean()
        loss.backward()
        return loss.detach().cpu(), q.grad, b.grad

    ch = _fit_curve(hip, q0.to(DEV), b0.to(DEV), steps, lr)
    dev32, dev = float(np.abs(c32 - c64).max()), float(np.abs(ch - c64).max())
    print(f"MANO-FIT f64 curve {c64.tolist()}  hip deviation {dev:.3e}  f32 restatement deviation {dev32:.3e}  gate {4 * dev32:.3e}")
    assert c64[-1] < 0.5 * c64[0]  # the fit makes progress
    assert dev32 > 0 and dev <= 4 * dev32


def test_rejected_arguments_launch_nothing():
    from oakink2_tamf_amd.hip_backend import _stream_ptr
    from oakink2_tamf_amd.mano import _bind

    lib, layer, N = _bind(), _layer(20, 0), 3
    q, b = _inputs(N)
    q, b = q.to(DEV), b.to(DEV)
    gv, gj = torch.ones(N, 20, 3, device=DEV), torch.ones(N, 21, 3, device=DEV)
    dq = torch.full((N, 16, 4), float("nan"), device=DEV)
    db = torch.full((N, 10), float("nan"), device=DEV)
    st = _stream_ptr(torch.device(DEV))
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    bad = {"both upstreams null": (layer._model, P(q), P(b), N, None, None, P(dq), P(db)),
           "negative N": (layer._model, P(q), P(b), -1, P(gv), P(gj), P(dq), P(db)),
           "null dquat_out": (layer._model, P(q), P(b), N, P(gv), P(gj), None, P(db)),
           "null model": (None, P(q), P(b), N, P(gv), P(gj), P(dq), P(db))}
    for name, args in bad.items():
        rc = lib.tamf_mano_backward(*args, st)
        assert rc == TAMF_ERR_INVALID, name
        assert lib.tamf_mano_last_error().decode(), name
        torch.cuda.synchronize()
        assert torch.isnan(dq).all() and torch.isnan(db).all(), name
    assert lib.tamf_mano_backward(layer._model, P(q), P(b), 0, P(gv), P(gj), P(dq), P(db), st) == 0  # N = 0: nothing is launched
    torch.cuda.synchronize()
    assert torch.isnan(dq).all() and torch.isnan(db).all()
    with pytest.raises(RuntimeError, match="upstream"):
        layer.backward_raw(q, b, None, None)
