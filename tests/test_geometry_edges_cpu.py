"""Conditions on the inputs of tests/geometry_cases.py, checked without a GPU: every reference is finite, every gate's e32 is
positive, every planted minimum is the float64 arg-min by a margin float32 cannot flip, every branch of the kernels is populated."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import geometry_cases as C  # noqa: E402
from oracle import geometry_oracle as G  # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)


def test_h2o_table_covers_the_stated_ranges():
    cases = C.H2O_CASES
    assert {1, 63, 64, 255, 256, 257, 778, 1023, 1024} <= {c[2] for c in cases}
    assert {c[4] for c in cases} == {1, 255, 256, 257, 513}
    assert {c[3] for c in cases} == {1, 3} and {c[1] for c in cases} == {1, 2, 5}
    for B, T, V, nobj, P, on in cases:
        assert B * T * V >= 64 and B * T >= 2
    kinds = set()
    for i in range(len(cases)):
        c = C.h2o_case(i)
        P = cases[i][4]
        for p in c["plants"]:
            if p[0] == "near":
                o, j = divmod(p[4], P)
                kinds |= {name for name, hit in (("first", j == 0), ("255", j == 255), ("256", j == 256), ("last", j == P - 1),
                                                 ("last_object", o > 0 and o == c["n_real"][p[1]] - 1)) if hit}
    assert kinds == {"first", "255", "256", "last", "last_object"}


@pytest.mark.parametrize("i", range(len(C.H2O_CASES)), ids=[C.h2o_id(c) for c in C.H2O_CASES])
def test_h2o_case_is_sound(i):
    B, T, V, nobj, P, _ = C.H2O_CASES[i]
    c = C.h2o_case(i)
    ref = c["ref"]
    assert ref.dtype == torch.float64 and ref.shape == (B, T, V) and bool(torch.isfinite(ref).all())
    print(f"h2o {C.h2o_id(C.H2O_CASES[i])}: e32 {c['e32']:.3e}, gate {C.GATE_FACTOR * c['e32']:.3e}")
    assert 0.0 < c["e32"] < 1e-6
    if c["obj_num"] is not None and min(c["n_real"]) < nobj:  # the padded objects are poison, and the reference did not read it
        assert bool(torch.isnan(c["traj"]).any()) and bool(torch.isnan(c["pts"]).any())
    else:
        assert not bool(torch.isnan(c["traj"]).any())
    assert all(1 <= n <= nobj for n in c["n_real"])
    kinds = [p[0] for p in c["plants"]]
    assert kinds.count("contact") == 1 and kinds.count("min") == 2 and (kinds.count("near") >= 1 or V * B * T <= 128)
    assert {p[3] for p in c["plants"] if p[0] == "min"} == {0, V - 1}
    for p in c["plants"]:
        b, t, v = p[1:4]
        d = C.h2o_frame(c, b, t)  # (V, n_real * P) float64, from the definition
        assert abs(d[v].min().item() - ref[b, t, v].item()) < 1e-12
        if p[0] == "near":
            assert int(d[v].argmin()) == p[4]
            if d.shape[1] > 1:
                assert d[v].topk(2, largest=False).values[1].item() - d[v].min().item() >= C.GAP
            assert 1e-3 < d[v].min().item() < 3e-3  # centimetres away from every other point, not a rounding
        elif p[0] == "min":
            per_vertex = d.min(dim=1).values
            assert int(per_vertex.argmin()) == v
            if V > 1:
                assert per_vertex.topk(2, largest=False).values[1].item() - per_vertex[v].item() >= C.GAP
        else:
            assert ref[b, t, v].item() == 0.0
            assert c["traj"][b, 0, t].tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0]
            o, j = divmod(int(d[v].argmin()), P)
            assert torch.equal(c["hand"][b, t, v], c["pts"][b, o, j])  # bit for bit
            # the float32 oracle gives exactly 0.0 there too
            assert G.h2o_dist(c["hand"][b:b + 1], c["traj"][b:b + 1], c["pts"][b:b + 1],
                              None if c["obj_num"] is None else c["obj_num"][b:b + 1])[0, t, v].item() == 0.0


def test_pose_truth_convention():
    """R(q) -> rot6d -> the float64 oracle gives q back: the constructed truth is the oracle's convention"""
    worst = 0.0
    for i in range(len(C.POSE_CASES)):
        c = C.pose_case(i)
        rng = np.random.default_rng(2000 + i)
        q, r6 = C._pose_rows(rng, c["N"] * c["J"])
        got = G.rotmat_to_quat(G.rot6d_to_rotmat(torch.from_numpy(r6))).numpy()
        worst = max(worst, float(C.quat_err(got, q).max()))
        assert np.array_equal(q.reshape(c["quat"].shape), c["quat"])
        assert np.abs(np.linalg.norm(q, axis=-1) - 1).max() < 1e-15 and (q[:, 0] >= 0).all()
    print(f"pose: float64 oracle against the constructed truth {worst:.3e}")
    assert worst < 5e-15


def test_pose_cases_are_sound():
    nj = [n * j for n, j in C.POSE_CASES]
    assert any(x % 256 == 0 for x in nj) and any(x % 256 and x > 256 for x in nj) and 257 in nj
    assert {n for n, _ in C.POSE_CASES} == {1, 255, 256, 257, 1000} and {j for _, j in C.POSE_CASES} == {1, 2, 16, 21}
    counts = np.zeros(4)
    for i, (N, J) in enumerate(C.POSE_CASES):
        c = C.pose_case(i)
        assert c["pose"].dtype == torch.float32 and c["pose"].shape == (N, 3 + 6 * J) and np.isfinite(c["quat"]).all()
        print(f"pose N{N}-J{J}: e32 {c['e32']:.3e}, gated with {C.pose_gate_e32(i):.3e} x {C.GATE_FACTOR}")
        assert 0.0 < c["e32"] < 1e-6 and c["e32"] <= C.pose_gate_e32(i) <= C.pose_e32_pooled()
        share = np.bincount(c["best"].reshape(-1), minlength=4) / (N * J)
        counts += np.bincount(c["best"].reshape(-1), minlength=4)
        if N * J >= 200:
            assert share.min() >= 0.05, (N, J, share)
            w = c["quat"].reshape(-1, 4)[:, 0]
            assert (w == 0.0).sum() >= 2 and (w == 1e-4).sum() >= 2  # the near-180-degree rows
    assert (counts / counts.sum()).min() >= 0.05
    assert 0.0 < C.pose_e32_pooled() < 1e-6


def test_pose_degenerate_rows():
    d = C.pose_degenerate()
    q32 = d["q32"]
    assert np.isfinite(d["pose"].numpy()).all()
    assert np.isfinite(q32).all() and (q32[..., 0] >= 0).all()  # what the kernel is held to, the oracle does itself
    q64 = C.oracle_quat(d["pose"].double(), 2).numpy()
    for name in C.DEGENERATE_WELL_CONDITIONED:  # the float32 oracle is a usable reference there: it agrees with its float64 self
        rows = d["kind"] == C.DEGENERATE_KINDS.index(name)
        err = float(np.abs(q32[rows] - q64[rows]).max())
        print(f"pose degenerate {name}: float32 oracle against float64 oracle {err:.3e}")
        assert err <= C.GATE_FACTOR * C.pose_e32_pooled(), name


@pytest.mark.parametrize("P", C.TRANSFORM_P)
def test_transform_case_is_sound(P):
    c = C.transform_case(P)
    assert len(c["calls"]) == len(C.TRANSFORM_T) * len(C.TRANSFORM_LEAD)
    assert sum(r.numel() for _, _, r in c["calls"]) >= 64
    for traj, pts, ref in c["calls"]:
        assert ref.dtype == torch.float64 and ref.shape == traj.shape[:-2] + (traj.shape[-2], P, 3) and bool(torch.isfinite(ref).all())
    print(f"transform P{P}: e32 {c['e32']:.3e}, gate {C.GATE_FACTOR * c['e32']:.3e}, float64 gate {C.transform_f64_gate(c['cmax']):.3e}")
    assert 0.0 < c["e32"] < 1e-6 and 0.01 < c["cmax"] < 2.0
    # the identity pose moves nothing, bit for bit, in either precision
    tr = torch.tensor(C.IDENTITY_TRAJ).repeat(2, 1)
    for dt in (torch.float32, torch.float64):
        p = c["calls"][0][1].to(dt).reshape(-1, 3)
        assert torch.equal(G.transform_points(tr.to(dt), p), p[None].expand(2, -1, -1))


@pytest.mark.parametrize("V,M", C.NORMALS_CASES)
def test_normals_case_is_sound(V, M):
    """the float32 oracle against a float64 evaluation of the definition.  A vertex's float32 sum carries the rounding of its
    terms: each edge difference and product is good to a few eps relative to |a| |b|, so the unnormalised sum is off by at most
    about 8 eps32 x sum |a| |b|; the normalisation divides by max(|n|, 1e-6) and adds a few eps of its own."""
    c = C.normals_case(V, M)
    assert c["faces"].shape == (max(2, 2 * V), 3) and c["faces"].min() >= 0 and c["faces"].max() < V
    f = c["faces"]
    assert (f[:, 0] == f[:, 2]).any()  # zero-area face
    assert len(np.unique(f, axis=0)) < len(f)  # duplicated face
    assert len(c["unref"]) >= (1 if V > 3 else 0)
    n64, ln, mag = C.normals_definition_f64(c["verts"], f)
    ref32 = c["ref32"]
    assert ref32.dtype == np.float32 and np.isfinite(ref32).all()
    assert (ref32[:, c["unref"]] == 0).all() and (n64[:, c["unref"]] == 0).all()
    bound = 16 * EPS32 * mag / np.maximum(ln, 1e-6) + 8 * EPS32
    err = np.abs(ref32 - n64).max(-1)
    print(f"normals V{V}-M{M}: float32 oracle against the float64 definition {err.max():.3e}, worst err / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    assert ln[-1].max() < 1e-6 < ln[0].max() or M == 1  # the scaled mesh takes the max(|x|, eps) branch, the others do not
    assert ln[-1].max() < 1e-6 and (np.linalg.norm(ref32[-1], axis=-1) < 0.99).all()


@pytest.mark.parametrize("subdiv,F", C.CONTAINS_MESHES)
def test_contains_cases_are_sound(subdiv, F):
    v, f = C.contains_mesh(subdiv, F)
    assert f.shape == (F, 3) and (f[:, 0] == f[:, 1]).sum() == F - 20 * 4 ** subdiv
    for N in C.CONTAINS_N:
        c = C.contains_case(subdiv, F, N)
        pts, ref = c["points"], c["ref"]
        assert ref.dtype == bool and ref.shape == (len(pts),) and len(pts) == N + 21
        # the padding faces change no boolean
        assert np.array_equal(ref, G.mesh_contains(v, f[: 20 * 4 ** subdiv], pts, C.RESOLUTION))
        if N >= 255:
            assert 0.1 < ref[:N].mean() < 0.9
        q = c["scale"] * pts + c["translate"]
        for ax, row in enumerate(c["at_res"]):
            assert q[row, ax] == C.RESOLUTION and not ref[row]
        assert not ref[N:].any()  # on the box, a hair outside, well outside: never inside the sphere
        assert ((q[N: N + 18] < 0) | (q[N: N + 18] > C.RESOLUTION)).any(axis=1).sum() == 6  # the six far points leave the rescaled frame
