"""CPU: what the MANO layer's edge tests stand on - the float64 restatement on the new axes (any tree, any fingertip ids, any joint
order, every centre) against facts that do not depend on it, finite differences under its autograd, the coverage of the case table
of tests/mano_cases.py - and the argument checks of the C entry points, called through ctypes: they return before any device call."""
import ctypes
import os
import sys
from ctypes import POINTER, c_double, c_int32, c_void_p

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import mano_cases as C  # noqa: E402
import mano_restatement as R  # noqa: E402

from oakink2_tamf_amd import mano as M  # noqa: E402

F64 = torch.float64
TAMF_ERR_INVALID = -1
DEFAULT_ORDER = list(M.DEFAULT_JOINT_ORDER)


def _identity(N):
    q = torch.zeros(N, 16, 4, dtype=F64)
    q[..., 0] = 1
    return q


def _descendants(par, j):
    desc = set()
    for k in range(16):
        p = k
        while p >= 0 and p != j:
            p = par[p]
        if p == j:
            desc.add(k)
    return desc


# ---- the restatement on the new axes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", C.TREES)
@pytest.mark.parametrize("V", [1, 17, 1024])
def test_identity_pose_zero_betas_is_the_template(tree, V):
    a = C.model(V, tree, "ends", "perm", seed=3)
    verts, joints, j16 = R.mano_forward(R.to_torch(a, F64), _identity(2), torch.zeros(2, 10, dtype=F64), center_idx=None)
    vt = torch.from_numpy(a.v_template)
    assert (verts - vt).abs().max() < 1e-14
    want = torch.from_numpy(a.J_regressor @ a.v_template)
    assert (j16 - want).abs().max() < 1e-14
    full = torch.cat([want, vt[a.tip_ids.tolist()]])[a.joint_order.tolist()]
    assert (joints - full).abs().max() < 1e-14


@pytest.mark.parametrize("tree", ["chain", "star", "rand"])
def test_rotating_a_joint_moves_exactly_its_descendants(tree):
    V = 64
    rng = np.random.default_rng(4)
    bound = np.concatenate([np.arange(16), rng.integers(0, 16, size=V - 16)])  # every joint has a vertex
    a = C.model(V, tree, "spread", "default", seed=1)
    a = M.ManoArrays(a.v_template, a.shapedirs, np.zeros((V, 3, 135)), a.J_regressor, np.eye(16)[bound], a.parents, a.faces,
                     tip_ids=a.tip_ids)
    par = a.parents.tolist()
    assert par == C.parents(tree, 1)
    m = R.to_torch(a, F64)
    betas = torch.from_numpy(rng.normal(size=(1, 10)))
    rest = R.mano_forward(m, _identity(1), betas, center_idx=None)[0]
    sizes = set()
    for j in range(16):
        q = _identity(1)
        q[0, j] = torch.tensor([0.6, 0.1, -0.7, 0.2], dtype=F64)
        moved = R.mano_forward(m, q, betas, center_idx=None)[0]
        desc = _descendants(par, j)
        sizes.add(len(desc))
        still = torch.from_numpy(~np.isin(bound, sorted(desc)))
        assert j in desc and (j != 0 or not still.any())
        if still.any():
            assert (moved[0][still] - rest[0][still]).abs().max() < 1e-14, (tree, j)
        assert (moved[0][~still] - rest[0][~still]).norm(dim=-1).min() > 1e-6, (tree, j)  # ... and every descendant's vertex does move
    assert 16 in sizes and 1 in sizes
    assert tree != "chain" or sizes == set(range(1, 17))
    assert tree != "star" or sizes == {1, 16}


@pytest.mark.parametrize("order", ["identity", "reversed", "perm"])
def test_joints_under_an_order_are_the_default_joints_permuted(order):
    V = 65
    base = C.model(V, "rand", "spread", "default", seed=2)
    P = C.joint_order(order, 2).tolist()
    other = M.ManoArrays(base.v_template, base.shapedirs, base.posedirs, base.J_regressor, base.weights, base.parents, base.faces,
                         tip_ids=base.tip_ids, joint_order=np.array(P))
    q, b = (t.double() for t in C.inputs(3, seed=1))
    v0, j0, _ = R.mano_forward(R.to_torch(base, F64), q, b, center_idx=None)
    v1, j1, _ = R.mano_forward(R.to_torch(other, F64), q, b, center_idx=None)
    assert torch.equal(v0, v1)
    # slot s of the default order shows source DEFAULT_ORDER[s]; under P slot s shows source P[s]
    where = [DEFAULT_ORDER.index(src) for src in P]
    assert torch.equal(j1, j0[:, where])
    assert order == "identity" or not torch.equal(j1, j0)


def test_duplicate_tips_give_identical_joint_rows():
    for V in (1, 2, 17):
        a = C.model(V, "mano", "ends", "perm", seed=5)
        assert a.tip_ids[0] == a.tip_ids[1] and a.tip_ids[2] == a.tip_ids[3]
        q, b = (t.double() for t in C.inputs(3, seed=2))
        v, j, _ = R.mano_forward(R.to_torch(a, F64), q, b, center_idx=None)
        slot = {int(src): s for s, src in enumerate(a.joint_order)}
        assert torch.equal(j[:, slot[16]], j[:, slot[17]]) and torch.equal(j[:, slot[18]], j[:, slot[19]])
        assert torch.equal(j[:, slot[16]], v[:, 0]) and torch.equal(j[:, slot[18]], v[:, V - 1])


@pytest.mark.parametrize("center", range(21))
def test_the_centre_row_is_zero_for_every_centre(center):
    a = C.model(65, "rand", "spread", "perm", seed=6)
    q, b = (t.double() for t in C.inputs(3, seed=3))
    m = R.to_torch(a, F64)
    v0, j0, _ = R.mano_forward(m, q, b, center_idx=None)
    v1, j1, _ = R.mano_forward(m, q, b, center_idx=center)
    assert float(j1[:, center].abs().max()) == 0.0
    assert (v0 - j0[:, center: center + 1] - v1).abs().max() < 1e-15 and (j0 - j0[:, center: center + 1] - j1).abs().max() < 1e-15
    src = int(a.joint_order[center])
    if src >= 16:  # a fingertip slot: that vertex sits at the origin
        assert float(v1[:, int(a.tip_ids[src - 16])].abs().max()) == 0.0


@pytest.mark.parametrize("tree", C.TREES)
def test_restatement_autograd_against_finite_differences(tree):
    """the yardstick of the gradient tests is float64 autograd through the restatement: held here to finite differences, through the
    normalisation (non-unit quaternions), a fingertip centre and duplicate tips"""
    a = C.model(17, tree, "ends", "perm", seed=7)
    center = [s for s in range(21) if a.joint_order[s] == 18][0]
    m = R.to_torch(a, F64)
    scale = np.where(np.arange(16) % 2 == 0, 0.5, 3.0)
    q, b = (torch.from_numpy(x).requires_grad_(True) for x in C.F.random_inputs(2, seed=4, scale=scale))
    assert torch.autograd.gradcheck(lambda q, b: R.mano_forward(m, q, b, center)[:2], (q, b), eps=1e-6, atol=1e-7, rtol=1e-5)


# ---- the case table -------------------------------------------------------------------------------------------------------------
def test_the_case_table_covers_what_it_claims():
    T = C.CASES
    assert 35 <= len(T) <= 45
    assert {c.V for c in T} == set(C.VS) and {c.tree for c in T} == set(C.TREES)
    assert {c.tips for c in T} == set(C.TIPS) and {c.order for c in T} == set(C.ORDERS)
    for V in C.VS:
        assert any(c.V == V and c.tree == "mano" and c.tips == "ends" for c in T), V
    for tree in C.TREES:
        for V in (1, 17, 1024):
            assert any(c.V == V and c.tree == tree for c in T), (tree, V)
    assert {c.center for c in T} == set(range(21)) | {None}
    on_chain = [c for c in T if c.order != "default" and c.center is not None and C.arrays(c).joint_order[c.center] < 16]
    on_tip = [c for c in T if c.order != "default" and c.center is not None and C.arrays(c).joint_order[c.center] >= 16]
    assert len(on_chain) >= 3 and len(on_tip) >= 3
    assert {c.order for c in on_tip} == {"identity", "reversed", "perm"}
    for V in (17, 1024):
        assert any(c.V == V and c.dense for c in T), V
    assert all(c.V == 778 for c in T if c.tips == "default")
    assert all(c.V >= 16 for c in T if c.tips == "one_tile")
    assert all(c.center is None for c in T if c.V == 1)  # (see mano_cases._table)


def test_the_models_are_what_the_axes_say():
    for c in C.CASES:
        a = C.arrays(c)
        par = a.parents.tolist()
        assert a.n_verts == c.V and par[0] == -1 and all(0 <= par[j] < j for j in range(1, 16))
        depth = [0] * 16
        for j in range(1, 16):
            depth[j] = depth[par[j]] + 1
        if c.tree != "rand":
            assert max(depth) == {"mano": 3, "chain": 15, "star": 1}[c.tree]
        tips = a.tip_ids.tolist()
        if c.tips == "ends":
            assert tips[:4] == [0, 0, c.V - 1, c.V - 1]
        if c.tips == "one_tile":
            assert len({t // 16 for t in tips}) == 1 and tips[0] // 16 == (c.V - 1) // 16 and c.V - 1 in tips
        if c.tips == "spread":
            assert len(set(tips)) == 5
        if c.order != "default":
            assert a.joint_order.tolist() != DEFAULT_ORDER
        nz = (a.weights != 0).sum(axis=1)
        if c.dense:
            assert (nz == 16).all() and (a.weights < 0).any() and (np.abs(a.weights.sum(axis=1) - 1) > 1e-3).all()
            assert (a.J_regressor != 0).all()
        else:
            assert nz.max() <= 4 and nz.min() >= 1 and np.abs(a.weights.sum(axis=1) - 1).max() < 1e-12
    assert C.parents("rand", 0) not in (C.parents("mano"), C.parents("chain"), C.parents("star"))


@pytest.mark.parametrize("c", C.CASES, ids=[C.case_id(c) for c in C.CASES])
def test_the_measured_gates_are_positive(c):
    """e32 > 0 for every case, forward and gradient: 4 * e32 is a gate and never a vacuous one, and the float64 yardstick is finite.
    The relative e32 of a gradient is float32 rounding (6e-8) over a few hundred terms; 1e-3 or more would mean that the float64
    gradient itself cancels to nothing (as dbetas of a centred V = 1 model does), where a relative gate is meaningless."""
    q, b, v64, j64, e32 = C.case_forward(c)
    assert q.shape == (C.N_FRAMES, 16, 4) and v64.shape == (C.N_FRAMES, c.V, 3) and torch.isfinite(v64).all() and torch.isfinite(j64).all()
    assert 0 < e32 < float("inf")
    _, _, gv, gj, dq64, db64, eq, eb = C.case_grad(c)
    assert torch.isfinite(dq64).all() and torch.isfinite(db64).all() and float(dq64.abs().max()) > 0 and float(db64.abs().max()) > 0
    assert 0 < eq < 1e-3 and 0 < eb < 1e-3


# ---- the C entry points' own argument checks ------------------------------------------------------------------------------------
def _lib():
    return M._bind()


def _create_args(V=17, seed=0):
    """valid arguments of tamf_mano_model_create as a dict of numpy arrays (kept alive by the caller) and scalars"""
    a = C.model(V, "mano", "ends", "perm", seed=seed)
    return dict(V=V, v_template=a.v_template.copy(), shapedirs=a.shapedirs.copy(), posedirs=a.posedirs.copy(),
                J_regressor=a.J_regressor.copy(), weights=a.weights.copy(), parents=a.parents.astype(np.int32),
                tip_ids=a.tip_ids.astype(np.int32), joint_order=a.joint_order.astype(np.int32), center_idx=0)


SENTINEL = 0x5A5A5A5A


def _create(d, model_out=True):
    """(status, message, *model_out or None) of one call; model_out starts as a sentinel, not NULL"""
    lib = _lib()

    def ptr(k, ct):
        return None if d[k] is None else np.ascontiguousarray(d[k]).ctypes.data_as(POINTER(ct))

    keep = {k: (None if d[k] is None else np.ascontiguousarray(d[k])) for k in d if k not in ("V", "center_idx")}
    d = dict(d, **keep)
    out = c_void_p(SENTINEL)
    rc = lib.tamf_mano_model_create(d["V"], ptr("v_template", c_double), ptr("shapedirs", c_double), ptr("posedirs", c_double),
                                    ptr("J_regressor", c_double), ptr("weights", c_double), ptr("parents", c_int32), ptr("tip_ids", c_int32),
                                    ptr("joint_order", c_int32), d["center_idx"], ctypes.byref(out) if model_out else None)
    return rc, lib.tamf_mano_last_error().decode(), out.value


def _rejected(d, names, **kw):
    rc, msg, out = _create(d, **kw)
    assert rc == TAMF_ERR_INVALID, (names, rc)
    assert msg and any(n in msg for n in ([names] if isinstance(names, str) else names)), (names, msg)
    if kw.get("model_out", True):
        assert out is None, (names, out)  # *model_out == NULL


@pytest.mark.parametrize("V", [0, 1025, -1])
def test_create_rejects_v_outside_the_range(V):
    d = _create_args()
    for k, per in (("v_template", 3), ("shapedirs", 30), ("posedirs", 405), ("J_regressor", 16), ("weights", 16)):
        d[k] = np.zeros(1025 * per)  # (long enough for whatever V the call might read)
    d.update(V=V, tip_ids=np.zeros(5, np.int32))
    _rejected(d, "V = %d" % V)


@pytest.mark.parametrize("center", [-2, 21])
def test_create_rejects_a_centre_outside_the_range(center):
    _rejected(dict(_create_args(), center_idx=center), "center_idx = %d" % center)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("name", ["v_template", "shapedirs", "posedirs", "J_regressor", "weights"])
def test_create_rejects_a_non_finite_value_and_names_the_array(name, bad):
    d = _create_args()
    d[name].reshape(-1)[-1] = bad  # the last element: the check reads the whole array
    _rejected(d, name)
    d = _create_args()
    d[name].reshape(-1)[0] = bad
    _rejected(d, name)


@pytest.mark.parametrize("what,j,p", [("a second root", 5, -1), ("a self-parent", 6, 6), ("a forward parent", 8, 9), ("parents[0] >= 0", 0, 0),
                                      ("parents[0] >= 0", 0, 3), ("a parent past the joints", 15, 16)])
def test_create_rejects_a_bad_tree(what, j, p):
    d = _create_args()
    d["parents"][j] = p
    _rejected(d, "parents[%d] = %d" % (j, p))


@pytest.mark.parametrize("i,t", [(0, -1), (4, 17), (2, 1 << 20)])
def test_create_rejects_a_tip_outside_the_vertices(i, t):
    d = _create_args(V=17)
    d["tip_ids"][i] = t
    _rejected(d, "tip_ids[%d] = %d" % (i, t))


@pytest.mark.parametrize("what,i,s", [("a repeat", 3, None), ("21", 0, 21), ("-1", 20, -1)])
def test_create_rejects_an_order_that_is_no_permutation(what, i, s):
    d = _create_args()
    d["joint_order"][i] = d["joint_order"][(i + 1) % 21] if s is None else s
    _rejected(d, "joint_order")


@pytest.mark.parametrize("name", ["v_template", "shapedirs", "posedirs", "J_regressor", "weights", "parents"])
def test_create_rejects_a_null_mandatory_pointer(name):
    _rejected(dict(_create_args(), **{name: None}), name)


def test_create_rejects_a_null_model_out():
    _rejected(_create_args(), "model_out", model_out=False)


def test_null_models_are_refused_everywhere_and_destroy_accepts_null():
    lib = _lib()
    assert lib.tamf_mano_model_destroy(None) == 0
    buf = (ctypes.c_float * 64)()  # never read: the model is checked first
    p = ctypes.addressof(buf)
    for name, rc in (("set_tiles", lib.tamf_mano_model_set_tiles(None, 1)),
                     ("forward", lib.tamf_mano_forward(None, p, p, 1, p, p, None)),
                     ("backward", lib.tamf_mano_backward(None, p, p, 1, p, p, p, p, None))):
        assert rc == TAMF_ERR_INVALID, name
        assert lib.tamf_mano_last_error().decode(), name
