"""GPU: the native MANO layer over what include/tamf_mano.h accepts - the case table of tests/mano_cases.py (V = 1 .. 1024 at the tile
edges, four kinematic trees, fingertips at vertex 0 / V - 1 / doubled / in one tile, four joint orders, every centre), the forward's
vertex-tile split at large N, the bits, guard bands around every output, edge inputs, non-finite frames, unaligned quaternions.

Tolerance: the rule of test_mano_gpu.py / test_mano_grad_gpu.py, neither re-chosen nor loosened.  Per case e32 is measured from the
float32 restatement against the float64 one on the case's own inputs (forward: max abs error over vertices and joints; gradients: per
tensor, max |g32 - g64| / max |g64|), and the HIP result must be within 4 * e32 of the float64 restatement."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import mano_cases as C  # noqa: E402
import mano_fixture as F  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAMF_ERR_INVALID = -1
_REF = {}
_WORST = {"forward": 0.0, "dquat": 0.0, "dbetas": 0.0}
IDS = [C.case_id(c) for c in C.CASES]


def _layer(a, center, differentiable=False):
    from oakink2_tamf_amd.mano import HipManoLayer

    key = ("layer", id(a), center, differentiable)
    if key not in _REF:
        _REF[key] = (a, HipManoLayer(a, center_idx=center, device=DEV, differentiable=differentiable))
    return _REF[key][1]


def _default_model():
    from oakink2_tamf_amd.mano import ManoArrays

    if "default" not in _REF:
        _REF["default"] = ManoArrays(**F.synthetic_arrays(778, 0))
    return _REF["default"]


def _dev(t):
    return None if t is None else t.to(DEV)


def _worst(name, ratio):
    _WORST[name] = max(_WORST[name], ratio)
    return _WORST[name]


def _tip_slots(a):
    slots = [s for s in range(21) if a.joint_order[s] >= 16]
    return slots, [int(a.tip_ids[a.joint_order[s] - 16]) for s in slots]


# ---- parity over the table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_forward_parity_over_the_table(c):
    q, b, v64, j64, e32 = C.case_forward(c)
    a, N = C.arrays(c), C.N_FRAMES
    layer = _layer(a, c.center)
    out = layer(pose_coeffs=q.to(DEV), betas=b.to(DEV))
    assert out.verts.shape == (N, c.V, 3) and out.joints.shape == (N, 21, 3) and out.verts.dtype == torch.float32
    ev = float((out.verts.cpu().double() - v64).abs().max())
    ej = float((out.joints.cpu().double() - j64).abs().max())
    ratio = max(ev, ej) / e32
    print(f"MANO-EDGE-PARITY {C.case_id(c)} N={N}: e32 {e32:.3e}  hip verts {ev:.3e} joints {ej:.3e}  gate {4 * e32:.3e}  "
          f"hip/e32 {ratio:.2f}  worst so far {_worst('forward', ratio):.2f}")
    assert np.isfinite(ev) and np.isfinite(ej) and e32 > 0
    assert ev <= 4 * e32 and ej <= 4 * e32
    only = layer.forward(q.to(DEV), b.to(DEV), with_joints=False)
    assert only.joints is None and torch.equal(only.verts, out.verts)  # joints_out NULL: the same vertex bits
    slots, tips = _tip_slots(a)
    assert len(slots) == 5 and torch.equal(out.joints[:, slots], out.verts[:, tips])  # the fingertip joints ARE the fingertip vertices
    if c.center is not None:
        assert float(out.joints[:, c.center].abs().max()) == 0.0


def _grad_check(tag, layer, ref, want_dbetas=True):
    q, b, gv, gj, dq64, db64, eq32, eb32 = ref
    dq, db = layer.backward_raw(q.to(DEV), b.to(DEV), _dev(gv), _dev(gj), want_dbetas=want_dbetas)
    assert dq.shape == tuple(q.shape) and dq.dtype == torch.float32 and dq.is_cuda
    eq = float((dq.cpu().double() - dq64).abs().max() / dq64.abs().max())
    eb = float("nan") if db is None else float((db.cpu().double() - db64).abs().max() / db64.abs().max())
    wb = _WORST["dbetas"] if db is None else _worst("dbetas", eb / eb32)
    print(f"MANO-EDGE-GRAD {tag}: dquat e32 {eq32:.3e} hip {eq:.3e} gate {4 * eq32:.3e} hip/e32 {eq / eq32:.2f} | dbetas e32 {eb32:.3e} "
          f"hip {eb:.3e} gate {4 * eb32:.3e} hip/e32 {eb / eb32:.2f} | worst so far {_worst('dquat', eq / eq32):.2f} {wb:.2f}")
    assert eq32 > 0 and eb32 > 0
    assert np.isfinite(eq) and eq <= 4 * eq32
    if want_dbetas:
        assert db.shape == (q.shape[0], 10) and np.isfinite(eb) and eb <= 4 * eb32
    else:
        assert db is None
    return dq, db


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_gradient_parity_over_the_table(c):
    _grad_check(C.case_id(c), _layer(C.arrays(c), c.center), C.case_grad(c))


VARIANT_MODELS = [c for c in C.CASES if (c.V, c.tree, c.tips) in ((1, "star", "ends"), (17, "rand", "spread"), (1024, "chain", "ends"))]


@pytest.mark.parametrize("which", ["verts", "joints", "nodbetas"])
@pytest.mark.parametrize("c", VARIANT_MODELS, ids=[C.case_id(c) for c in VARIANT_MODELS])
def test_gradient_variants(c, which):
    """upstream on the vertices only, on the joints only, and dbetas_out NULL (the same dquat bits)"""
    assert len(VARIANT_MODELS) == 3
    layer = _layer(C.arrays(c), c.center)
    ref = C.case_grad(c, "both" if which == "nodbetas" else which)
    dq, _ = _grad_check(f"{C.case_id(c)} {which}", layer, ref, want_dbetas=which != "nodbetas")
    if which == "nodbetas":
        q, b, gv, gj = ref[:4]
        assert torch.equal(layer.backward_raw(q.to(DEV), b.to(DEV), _dev(gv), _dev(gj))[0], dq)


# ---- the forward's vertex-tile split --------------------------------------------------------------------------------------------
def _launch_shape(V, N, m_tiles=1):
    """(gy, tiles_per_group, tiles of the last group) as tamf_mano_forward derives them (csrc/tamf_mano.hip): nx = ceil(N / (16 mt)),
    gy = clamp(ceil(1024 / nx), 1, ceil(ntiles / 4)), tiles_per_group = ceil(ntiles / gy), gy = ceil(ntiles / tiles_per_group)"""
    ntiles = (V + 15) // 16
    nx = -(-N // (16 * m_tiles))
    gy = max(1, min(-(-1024 // nx), (ntiles + 3) // 4))
    tpg = -(-ntiles // gy)
    gy = -(-ntiles // tpg)
    return gy, tpg, ntiles - (gy - 1) * tpg


# (V, N, m_tiles, what the formula above gives: gy, tiles per group, tiles of the last group)
SPLITS = [(1024, 1104, 0, (13, 5, 4)),     # five tiles per group: wave 0 runs a second round
          (1024, 1104, 4, (16, 4, 4)),     # the same batch with four frame tiles per workgroup
          (1024, 5472, 0, (3, 22, 20)),    # an intermediate split with a short last group
          (778, 5472, 0, (3, 17, 15)),
          (778, 16385, 0, (1, 49, 49)),    # gy = 1: one workgroup walks every tile
          (1024, 16385, 0, (1, 64, 64))]


def _split_base(V):
    """the N = 33 call every frame of the large batches is compared with; itself held to the float64 gate"""
    key = ("split", V)
    if key not in _REF:
        c = [c for c in C.CASES if c.V == V and c.tree == "mano" and c.tips == "ends"][0]
        a = C.arrays(c)
        q, b = C.inputs(33, seed=50 + V)
        v64, j64, e32 = C.forward_reference(a, c.center, q, b)
        layer = _layer(a, c.center)
        out = layer(pose_coeffs=q.to(DEV), betas=b.to(DEV))
        assert _launch_shape(V, 33)[1] == 4  # the shape every N <= 33 launch has
        ev, ej = float((out.verts.cpu().double() - v64).abs().max()), float((out.joints.cpu().double() - j64).abs().max())
        assert e32 > 0 and ev <= 4 * e32 and ej <= 4 * e32
        _REF[key] = (layer, q.to(DEV), b.to(DEV), out)
    return _REF[key]


@pytest.mark.parametrize("V,N,tiles,shape", SPLITS, ids=[f"V{V}-N{N}-t{t}" for V, N, t, _ in SPLITS])
def test_vertex_tile_split_does_not_change_a_bit(V, N, tiles, shape):
    assert _launch_shape(V, N, tiles or 1) == shape
    layer, q, b, base = _split_base(V)
    idx = torch.arange(N, device=DEV) % 33  # 33 distinct frames repeated
    try:
        layer.set_tiles(tiles)
        out = layer(pose_coeffs=q[idx], betas=b[idx])
    finally:
        layer.set_tiles(0)
    assert out.verts.shape == (N, V, 3)
    for k in range(33):  # (frame by frame: no second N x V x 3 tensor)
        sel = torch.arange(k, N, 33, device=DEV)
        assert bool((out.verts[sel] == base.verts[k]).all()) and bool((out.joints[sel] == base.joints[k]).all()), k
    assert torch.isfinite(base.verts).all()  # (== on finite values is bit equality up to the sign of zero, which no path here changes)


# ---- bits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", ["chain", "star"])
@pytest.mark.parametrize("V", [1, 16, 17, 65, 1024])
def test_bits_do_not_depend_on_batch_position_tiles_or_stream(V, tree):
    a = C.model(V, tree, "ends", "perm", seed=11)
    layer = _layer(a, 8)
    q, b = C.inputs(33, seed=V)
    gv, gj = C.upstream(V, 33, V)
    q, b, gv, gj = q.to(DEV), b.to(DEV), gv.to(DEV), gj.to(DEV)
    full = layer(pose_coeffs=q, betas=b)
    fq, fb = layer.backward_raw(q, b, gv, gj)
    assert torch.isfinite(full.verts).all() and torch.isfinite(fq).all() and torch.isfinite(fb).all() and float(fq.abs().max()) > 0

    def same(out, dq, db, sl, what):
        assert torch.equal(out.verts, full.verts[sl]) and torch.equal(out.joints, full.joints[sl]), what
        assert torch.equal(dq, fq[sl]) and torch.equal(db, fb[sl]), what

    def run(sl):
        return (layer(pose_coeffs=q[sl], betas=b[sl]),) + layer.backward_raw(q[sl], b[sl], gv[sl], gj[sl])

    for k in (0, 15, 16, 32):  # a frame alone
        same(*run(slice(k, k + 1)), slice(k, k + 1), ("alone", k))
    for n in (1, 15, 16, 17):  # the first n frames as a batch of n
        same(*run(slice(0, n)), slice(0, n), ("batch", n))
    try:
        for tiles in (1, 2, 4):
            layer.set_tiles(tiles)
            same(*run(slice(0, 33)), slice(0, 33), ("tiles", tiles))
    finally:
        layer.set_tiles(0)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        res = run(slice(0, 33))
    side.synchronize()
    same(*res, slice(0, 33), "stream")


# ---- guard bands ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 17])
@pytest.mark.parametrize("V", [1, 17, 1009])
def test_outputs_stay_inside_their_buffers(V, N):
    """the four outputs carved out of larger sentinel-filled tensors, NaN inside: the surroundings are untouched, every element inside is
    overwritten, and the values are the wrapper's"""
    from oakink2_tamf_amd.hip_backend import _stream_ptr
    from oakink2_tamf_amd.mano import _bind

    lib, st = _bind(), _stream_ptr(torch.device(DEV))
    a = C.model(V, "rand", "ends", "reversed", seed=13)
    layer = _layer(a, 20)
    q, b = C.inputs(N, seed=3)
    gv, gj = C.upstream(V, N, 3)
    q, b, gv, gj = q.to(DEV), b.to(DEV), gv.to(DEV), gj.to(DEV)
    PAD, SENT = 4096, -7.5
    sizes = {"verts": N * V * 3, "joints": N * 21 * 3, "dquat": N * 64, "dbetas": N * 10}
    big = {k: torch.full((2 * PAD + n,), SENT, device=DEV) for k, n in sizes.items()}
    inner = {k: big[k][PAD: PAD + n] for k, n in sizes.items()}
    for t in inner.values():
        t.fill_(float("nan"))
    assert inner["dquat"].data_ptr() % 16 == 0
    assert lib.tamf_mano_forward(layer._model, q.data_ptr(), b.data_ptr(), N, inner["verts"].data_ptr(), inner["joints"].data_ptr(), st) == 0
    assert lib.tamf_mano_backward(layer._model, q.data_ptr(), b.data_ptr(), N, gv.data_ptr(), gj.data_ptr(), inner["dquat"].data_ptr(),
                                  inner["dbetas"].data_ptr(), st) == 0
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert bool((big[k][:PAD] == SENT).all()) and bool((big[k][PAD + n:] == SENT).all()), k
        assert not bool(torch.isnan(inner[k]).any()), k
    want = layer(pose_coeffs=q, betas=b)  # (after the surroundings were checked: the wrapper's outputs have no band around them)
    want_q, want_b = layer.backward_raw(q, b, gv, gj)
    assert torch.equal(inner["verts"].view(N, V, 3), want.verts) and torch.equal(inner["joints"].view(N, 21, 3), want.joints)
    assert torch.equal(inner["dquat"].view(N, 16, 4), want_q) and torch.equal(inner["dbetas"].view(N, 10), want_b)


# ---- edge inputs ----------------------------------------------------------------------------------------------------------------
def _edge_run(tag, q, b, per_joint):
    """V = 778, the default model, centre 0: forward within the gate; gradients within the gate - per tensor, or (`per_joint`) dquat per
    joint with error and e32 both relative to that joint's largest |g64|.  Returns (out, dq, db, dq64)."""
    a, N = _default_model(), q.shape[0]
    layer = _layer(a, 0)
    v64, j64, e32 = C.forward_reference(a, 0, q, b)
    out = layer(pose_coeffs=q.to(DEV), betas=b.to(DEV))
    ev, ej = float((out.verts.cpu().double() - v64).abs().max()), float((out.joints.cpu().double() - j64).abs().max())
    print(f"MANO-EDGE-INPUT {tag}: forward e32 {e32:.3e} hip verts {ev:.3e} joints {ej:.3e} gate {4 * e32:.3e}")
    assert e32 > 0 and np.isfinite(ev) and np.isfinite(ej) and ev <= 4 * e32 and ej <= 4 * e32
    gv, gj = C.upstream(778, N, 77)
    dq64, db64 = C.restatement_grads(a, 0, q, b, gv, gj, torch.float64)
    dq32, db32 = C.restatement_grads(a, 0, q, b, gv, gj, torch.float32)
    dq, db = layer.backward_raw(q.to(DEV), b.to(DEV), gv.to(DEV), gj.to(DEV))
    assert torch.isfinite(dq).all() and torch.isfinite(db).all()
    dqc = dq.cpu().double()
    eb32, eb = float((db32 - db64).abs().max() / db64.abs().max()), float((db.cpu().double() - db64).abs().max() / db64.abs().max())
    print(f"MANO-EDGE-INPUT {tag}: dbetas e32 {eb32:.3e} hip {eb:.3e} gate {4 * eb32:.3e}")
    assert eb32 > 0 and eb <= 4 * eb32
    if per_joint:
        for j in range(16):
            top = float(dq64[:, j].abs().max())
            if top == 0.0:  # (a zero quaternion: its row is asserted exactly zero by the caller)
                continue
            e32j, ej = float((dq32[:, j] - dq64[:, j]).abs().max()) / top, float((dqc[:, j] - dq64[:, j]).abs().max()) / top
            print(f"MANO-EDGE-INPUT {tag}: dquat joint {j} max |g64| {top:.3e} e32 {e32j:.3e} hip {ej:.3e} gate {4 * e32j:.3e}")
            assert e32j > 0 and ej <= 4 * e32j, j
    else:
        eq32, eq = float((dq32 - dq64).abs().max() / dq64.abs().max()), float((dqc - dq64).abs().max() / dq64.abs().max())
        print(f"MANO-EDGE-INPUT {tag}: dquat e32 {eq32:.3e} hip {eq:.3e} gate {4 * eq32:.3e}")
        assert eq32 > 0 and eq <= 4 * eq32
    return out, dq, db, dq64


def test_a_zero_quaternion_is_the_identity_rotation():
    q, b = C.inputs(33, seed=61)
    q[:, 5] = 0.0   # a mid-chain joint in every frame
    q[4, 0] = 0.0   # the root of one frame
    q[9, 15] = 0.0  # a leaf of another
    out, dq, db, dq64 = _edge_run("zero quaternion", q, b, per_joint=False)
    zero = q.abs().sum(-1) == 0
    assert int(zero.sum()) == 35 and float(dq64[zero].abs().max()) == 0.0  # (the yardstick agrees: no gradient through the clamp at 0)
    assert float(dq[zero.to(DEV)].abs().max()) == 0.0
    assert float(dq[~zero.to(DEV)].abs().max()) > 0
    qi = q.clone()
    qi[zero] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    same = _layer(_default_model(), 0)(pose_coeffs=qi.to(DEV), betas=b.to(DEV))
    assert torch.equal(same.verts, out.verts) and torch.equal(same.joints, out.joints)


@pytest.mark.parametrize("lo,hi", [(1e-13, 1e-11), (1e-18, 1e18)], ids=["either-side-of-the-clamp", "1e-18-and-1e18"])
def test_quaternion_lengths_around_the_clamp_and_far_from_it(lo, hi):
    """|q| = lo on joints 2 and 12, hi on joints 0 and 7, 1 elsewhere: below the clamp (1e-12) the layer divides by the constant and the
    gradient has no projection; the rows differ by up to 1e36, so dquat is gated per joint.  The squares stay inside float32."""
    scale = np.ones(16)
    scale[[2, 12]], scale[[0, 7]] = lo, hi
    q, b = C.inputs(33, seed=62, scale=scale)
    n = q.double().norm(dim=-1)
    assert float((n[:, 2] / lo - 1).abs().max()) < 1e-6 and float((n[:, 7] / hi - 1).abs().max()) < 1e-6
    assert not (0.5e-12 < lo < 2e-12) and not (0.5e-12 < hi < 2e-12) and hi * hi < 3.4e38 and lo * lo > 1.2e-38
    _edge_run(f"|q| {lo:g} / {hi:g}", q, b, per_joint=True)


def test_large_betas():
    q, b = C.inputs(33, seed=63)
    b = torch.where(b > 0, 30.0, -30.0)
    _edge_run("betas +-30", q, b, per_joint=False)


# ---- non-finite isolation -------------------------------------------------------------------------------------------------------
def test_a_non_finite_frame_spoils_only_itself():
    """frames 3 (NaN in a quaternion), 20 (+Inf in a beta) and 31 (NaN in its dverts) of a batch of 33: every other frame's four outputs
    keep the bits of the clean batch, although the 16 frames of a tile share MFMA operands.  (Ordinary float values; nothing faults.)"""
    a = _default_model()
    layer = _layer(a, 0)
    q, b = C.inputs(33, seed=64)
    gv, gj = C.upstream(778, 33, 64)
    q, b, gv, gj = q.to(DEV), b.to(DEV), gv.to(DEV), gj.to(DEV)
    clean = layer(pose_coeffs=q, betas=b)
    cq, cb = layer.backward_raw(q, b, gv, gj)
    assert all(bool(torch.isfinite(t).all()) for t in (clean.verts, clean.joints, cq, cb))
    pq, pb, pgv = q.clone(), b.clone(), gv.clone()
    pq[3, 6, 2] = float("nan")
    pb[20, 4] = float("inf")
    pgv[31, 400, 1] = float("nan")
    out = layer(pose_coeffs=pq, betas=pb)
    dq, db = layer.backward_raw(pq, pb, pgv, gj)
    keep_f = torch.tensor([k not in (3, 20) for k in range(33)], device=DEV)  # (the forward does not see dverts)
    keep_b = torch.tensor([k not in (3, 20, 31) for k in range(33)], device=DEV)
    assert torch.equal(out.verts[keep_f], clean.verts[keep_f]) and torch.equal(out.joints[keep_f], clean.joints[keep_f])
    assert torch.equal(dq[keep_b], cq[keep_b]) and torch.equal(db[keep_b], cb[keep_b])
    assert not bool(torch.isfinite(out.verts[3]).all()) and not bool(torch.isfinite(out.verts[20]).all())  # (the poison did arrive)
    assert not bool(torch.isfinite(dq[31]).all())


# ---- alignment ------------------------------------------------------------------------------------------------------------------
def test_the_c_calls_refuse_a_quaternion_pointer_off_16_bytes():
    from oakink2_tamf_amd.hip_backend import _stream_ptr
    from oakink2_tamf_amd.mano import _bind

    lib, st, N, V = _bind(), _stream_ptr(torch.device(DEV)), 3, 17
    layer = _layer(C.model(V, "mano", "ends", "default", seed=14), 0)
    qbuf = torch.zeros(N * 64 + 4, device=DEV)
    dqbuf = torch.full((N * 64 + 4,), float("nan"), device=DEV)
    b, gv, gj = torch.zeros(N, 10, device=DEV), torch.ones(N, V, 3, device=DEV), torch.ones(N, 21, 3, device=DEV)
    verts, joints = torch.full((N, V, 3), float("nan"), device=DEV), torch.full((N, 21, 3), float("nan"), device=DEV)
    db = torch.full((N, 10), float("nan"), device=DEV)
    assert qbuf.data_ptr() % 16 == 0 and dqbuf.data_ptr() % 16 == 0
    calls = {"forward, quat": lambda: lib.tamf_mano_forward(layer._model, qbuf.data_ptr() + 4, b.data_ptr(), N, verts.data_ptr(), joints.data_ptr(), st),
             "backward, quat": lambda: lib.tamf_mano_backward(layer._model, qbuf.data_ptr() + 4, b.data_ptr(), N, gv.data_ptr(), gj.data_ptr(),
                                                              dqbuf.data_ptr(), db.data_ptr(), st),
             "backward, dquat_out": lambda: lib.tamf_mano_backward(layer._model, qbuf.data_ptr(), b.data_ptr(), N, gv.data_ptr(), gj.data_ptr(),
                                                                   dqbuf.data_ptr() + 4, db.data_ptr(), st)}
    for name, call in calls.items():
        assert call() == TAMF_ERR_INVALID, name
        assert "16-byte aligned" in lib.tamf_mano_last_error().decode(), name
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (verts, joints, dqbuf, db)), name  # nothing was launched


def test_the_layer_accepts_a_contiguous_view_off_16_bytes():
    """a contiguous (N, 16, 4) view that starts one float into its buffer: the bits of an aligned copy - forward, backward_raw and through
    autograd (the layer copies such an input; the C entry points refuse it)"""
    V, N = 17, 19
    a = C.model(V, "rand", "spread", "perm", seed=15)
    plain, diff = _layer(a, 3), _layer(a, 3, differentiable=True)
    q, b = C.inputs(N, seed=65)
    gv, gj = C.upstream(V, N, 65)
    q, b, gv, gj = q.to(DEV), b.to(DEV), gv.to(DEV), gj.to(DEV)
    buf = torch.zeros(N * 64 + 1, device=DEV)
    off = buf[1:].view(N, 16, 4)
    off.copy_(q)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4 and q.data_ptr() % 16 == 0 and torch.equal(off, q)
    want = plain(pose_coeffs=q, betas=b)
    want_q, want_b = plain.backward_raw(q, b, gv, gj)
    got = plain(pose_coeffs=off, betas=b)
    assert torch.equal(got.verts, want.verts) and torch.equal(got.joints, want.joints)
    got_q, got_b = plain.backward_raw(off, b, gv, gj)
    assert torch.equal(got_q, want_q) and torch.equal(got_b, want_b)
    qg, bg = off.detach().requires_grad_(True), b.clone().requires_grad_(True)
    assert qg.data_ptr() % 16 == 4
    out = diff(pose_coeffs=qg, betas=bg)
    assert torch.equal(out.verts, want.verts) and torch.equal(out.joints, want.joints)
    ((out.verts * gv).sum() + (out.joints * gj).sum()).backward()
    assert torch.equal(qg.grad, want_q) and torch.equal(bg.grad, want_b)
