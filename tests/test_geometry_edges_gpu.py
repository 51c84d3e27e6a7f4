"""GPU: the geometry kernels of csrc/tamf_geom.h over their accepted shape ranges, against the float64 references and planted edge
inputs of tests/geometry_cases.py (whose soundness tests/test_geometry_edges_cpu.py checks without a GPU); the bits that must not
depend on the batch; outputs carved out of sentinel-filled buffers; refused arguments.

What each group of cases would catch:
  h2o, P in {1, 255, 257, 513} with the nearest point planted at j = 0 / 255 / 256 / P - 1: a tile loop that drops or repeats the
      partial tile (`p0 + 256 <= P` for `p0 < P`), a padding point that wins, an off-by-one at the tile seam - errors of 1e-3 and more
  h2o, V in {1 .. 1024} with the frame minimum planted at v = 0 and v = V - 1: a register slot or a wave left out of the frame_min
      fold, a wave without vertices whose 3e38 leaks into it, a slot bound `v <= V`
  h2o, ragged obj_num over NaN-filled padding objects: a loop over nobj instead of obj_num[b], an object stride taken from obj_num
  pose, four branches each >= 5 % of the rows, compared with their sign where |w| >= 1e-3: a wrong sign or index in one branch
  pose / normals / transform at N J, n_mesh V, P off the 256-thread block: a tail that is dropped or runs over (sentinel test)
  contains at F = 64 / 65 / 128 / 129 and N = 255 / 256 / 257: a last LDS tile of one triangle that is skipped or read past F
"""
import os
import sys
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import geometry_cases as C  # noqa: E402
from oracle import geometry_oracle as G  # noqa: E402

pytestmark = pytest.mark.gpu

# Gates: GATE_FACTOR x e32 of the case for the float32 kernels (e32 = float32 oracle on the CPU against the float64 reference, never a
# kernel's own figure; it moves by up to 1.5x between CPUs), 64 eps64 x max |coordinate| for transform_points<double>, 2e-7 against the
# float32 oracle for the vertex normals (same summation order, no contraction), exact booleans for mesh_contains.  Measured over the
# tables (the tests print every case; "worst ratio" = the largest HIP error / e32 of one case, to be held against GATE_FACTOR):
#                          e32 (CPU float32)        HIP on MI355X            worst ratio
#   h2o_dist               1.4e-08 .. 1.7e-07       1.4e-08 .. 1.5e-07       1.37 (V 256, P 513)
#   h2o_dist, B = 65535    8.8e-08                  (inputs re-conditioned after the recorded run: 2.9e-06 of 3.8e-06 before)
#   pose decode            4.9e-08 .. 1.7e-07       4.9e-08 .. 1.5e-07       1.17 (N 256, J 2)
#   pose, degenerate rows  against the float32 oracle: 6.0e-08 (a1 = 0, a2 = 0, scale 1e15), gate 6.6e-07
#   transform<float>       3.6e-08 .. 1.3e-07       2.4e-08 .. 1.4e-07       1.34 (P 257)
#   transform<double>      gate 4.5e-15 .. 6.9e-15  5.6e-17 .. 2.9e-16
#   vertex normals         gate 2e-7                0 in all 15 cases (the same bits as the float32 oracle)
#   mesh_contains          exact                    equal in all 16 (mesh, N) cases
# No kernel needs more than the 4x: the fmaf chains of h2o_dist, pose decode and transform<float> against torch's separate multiplies and
# adds stay within 1.4x of e32.
GATE_FACTOR = C.GATE_FACTOR
SENTINEL = -3.0
PAD = 4096
INVALID = -1  # TAMF_ERR_INVALID


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint64)


def _geometry():
    from oakink2_tamf_amd import geometry

    return geometry


def _raw(entry, *args):
    """the C entry point itself with the current stream appended -> (rc, message)"""
    from oakink2_tamf_amd import hip_backend as hb

    L = _geometry()._bind()
    rc = getattr(L, entry)(*[c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args],
                           c_void_p(hb._stream_ptr(torch.device("cuda", torch.cuda.current_device()))))
    torch.cuda.synchronize()
    return rc, (L.tamf_last_error(None) or b"").decode()


def _carved(n, dtype=torch.float32):
    big = torch.full((2 * PAD + n,), SENTINEL, device="cuda", dtype=dtype)
    return big, big[PAD: PAD + n]


def _untouched_and_full(big, n):
    assert bool((big[:PAD] == SENTINEL).all()) and bool((big[PAD + n:] == SENTINEL).all())  # the surroundings
    assert bool((big[PAD: PAD + n] != SENTINEL).all())  # every element inside was written


# ---- parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(C.H2O_CASES)), ids=[C.h2o_id(c) for c in C.H2O_CASES])
def test_h2o_parity(i):
    geometry = _geometry()
    c = C.h2o_case(i)
    hv, tr, pts = c["hand"].cuda(), c["traj"].cuda(), c["pts"].cuda()
    got = geometry.multi_object_h2o_dist(hv, tr, pts, c["obj_num"])
    fmin = geometry.contact_min_dist(hv, tr, pts, c["obj_num"])
    assert got.shape == c["ref"].shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    err = float((got.cpu().double() - c["ref"]).abs().max())
    gate = GATE_FACTOR * c["e32"]
    print(f"h2o {C.h2o_id(C.H2O_CASES[i])}: HIP {err:.3e}, CPU float32 e32 {c['e32']:.3e}, gate {gate:.3e}")
    assert err <= gate
    assert torch.equal(fmin, got.min(dim=-1).values)  # the frame minimum is the minimum of the same values, bit for bit
    err_min = float((fmin.cpu().double() - c["ref"].min(dim=-1).values).abs().max())
    assert err_min <= gate
    for p in c["plants"]:
        b, t, v = p[1:4]
        if p[0] == "contact":
            assert got[b, t, v].item() == 0.0 and fmin[b, t].item() == 0.0
        elif p[0] == "min":
            assert int(got[b, t].argmin()) == v and fmin[b, t].item() == got[b, t, v].item()


@pytest.mark.parametrize("i", range(len(C.POSE_CASES)), ids=[f"N{n}-J{j}" for n, j in C.POSE_CASES])
def test_pose_parity(i):
    geometry = _geometry()
    c = C.pose_case(i)
    tsl, quat = geometry.pose_repr_to_quat(c["pose"].cuda())
    assert quat.shape == c["quat"].shape and tsl.shape == (c["N"], 3)
    assert np.array_equal(bits(tsl), bits(c["pose"][:, :3]))
    q = quat.cpu().numpy()
    assert np.isfinite(q).all() and (q[..., 0] >= 0).all()
    err = float(C.quat_err(q, c["quat"]).max())
    e32 = C.pose_gate_e32(i)
    print(f"pose N{c['N']}-J{c['J']}: HIP {err:.3e}, CPU float32 e32 {c['e32']:.3e} (gated with {e32:.3e}), gate {GATE_FACTOR * e32:.3e}")
    assert err <= GATE_FACTOR * e32


def test_pose_degenerate_rows():
    geometry = _geometry()
    d = C.pose_degenerate()
    tsl, quat = geometry.pose_repr_to_quat(d["pose"].cuda())
    assert np.array_equal(bits(tsl), bits(d["pose"][:, :3]))
    q = quat.cpu().numpy()
    assert np.isfinite(q).all() and (q[..., 0] >= 0).all()
    gate = GATE_FACTOR * C.pose_e32_pooled()
    for name in C.DEGENERATE_WELL_CONDITIONED:
        rows = d["kind"] == C.DEGENERATE_KINDS.index(name)
        err = float(np.abs(q[rows].astype(np.float64) - d["q32"][rows]).max())
        print(f"pose degenerate {name}: HIP against the float32 oracle {err:.3e}, gate {gate:.3e}")
        assert err <= gate, name


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("P", C.TRANSFORM_P)
def test_transform_parity(P, dtype):
    geometry = _geometry()
    c = C.transform_case(P)
    gate = GATE_FACTOR * c["e32"] if dtype == torch.float32 else C.transform_f64_gate(c["cmax"])
    err = 0.0
    for traj, pts, ref in c["calls"]:
        got = geometry.transform_points(traj.to(dtype).cuda(), pts.to(dtype).cuda())
        assert got.dtype == dtype and got.shape == ref.shape
        err = max(err, float((got.cpu().double() - ref).abs().max()))
    print(f"transform P{P} {dtype}: HIP {err:.3e}, CPU float32 e32 {c['e32']:.3e}, gate {gate:.3e}")
    assert err <= gate
    # the identity pose moves nothing, bit for bit
    p = c["calls"][-1][1].to(dtype).cuda()  # (2, 3, P, 3)
    tr = torch.tensor(C.IDENTITY_TRAJ, dtype=dtype).expand(2, 3, 3, 9).cuda()
    assert np.array_equal(bits(geometry.transform_points(tr, p)), bits(p[:, :, None].expand(2, 3, 3, P, 3)))


@pytest.mark.parametrize("V,M", C.NORMALS_CASES)
def test_normals_parity(V, M):
    geometry = _geometry()
    c = C.normals_case(V, M)
    got = geometry.vertex_normals(torch.from_numpy(c["verts"]).cuda(), c["faces"]).cpu().numpy()
    assert got.shape == c["ref32"].shape and np.isfinite(got).all()
    err = float(np.abs(got - c["ref32"]).max())
    print(f"normals V{V}-M{M}: HIP against the float32 oracle {err:.3e}, gate 2e-7")
    assert err <= 2e-7
    assert (got[:, c["unref"]] == 0).all()  # a vertex without a face: exactly 0


@pytest.mark.parametrize("subdiv,F", C.CONTAINS_MESHES)
def test_contains_parity(subdiv, F):
    geometry = _geometry()
    for N in C.CONTAINS_N:
        c = C.contains_case(subdiv, F, N)
        got = geometry.mesh_contains(c["verts"], c["faces"], torch.from_numpy(c["points"]).cuda(), C.RESOLUTION)
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), c["ref"]), (F, N)


# ---- bits ---------------------------------------------------------------------------------------------------------------------
RAGGED = [i for i, c in enumerate(C.H2O_CASES) if c[0] == 3 and c[5] is not None]


@pytest.mark.parametrize("i", RAGGED, ids=[C.h2o_id(C.H2O_CASES[i]) for i in RAGGED])
def test_h2o_rows_do_not_depend_on_the_batch(i):
    geometry = _geometry()
    c = C.h2o_case(i)
    hv, tr, pts, on = c["hand"].cuda(), c["traj"].cuda(), c["pts"].cuda(), c["obj_num"]
    batch = geometry.multi_object_h2o_dist(hv, tr, pts, on)
    fmin = geometry.contact_min_dist(hv, tr, pts, on)
    assert np.array_equal(bits(geometry.multi_object_h2o_dist(hv, tr, pts, on)), bits(batch))  # the same call twice
    assert np.array_equal(bits(geometry.contact_min_dist(hv, tr, pts, on)), bits(fmin))
    assert np.array_equal(bits(fmin), bits(batch.min(dim=-1).values))
    for b in range(3):  # a clip alone (B = 1)
        s = slice(b, b + 1)
        assert np.array_equal(bits(geometry.multi_object_h2o_dist(hv[s], tr[s], pts[s], on[s])), bits(batch[s])), b
        assert np.array_equal(bits(geometry.contact_min_dist(hv[s], tr[s], pts[s], on[s])), bits(fmin[s])), b
    perm = [2, 0, 1]
    onp = [on[b] for b in perm]
    assert np.array_equal(bits(geometry.multi_object_h2o_dist(hv[perm], tr[perm], pts[perm], onp)), bits(batch[perm]))
    assert np.array_equal(bits(geometry.contact_min_dist(hv[perm], tr[perm], pts[perm], onp)), bits(fmin[perm]))


def test_pose_batched_shape_is_the_flattened_call():
    geometry = _geometry()
    i = C.POSE_CASES.index((1000, 16))
    pose = C.pose_case(i)["pose"].cuda()
    tsl, quat = geometry.pose_repr_to_quat(pose)
    tsl3, quat3 = geometry.pose_repr_to_quat(pose.reshape(8, 125, 99))
    assert quat3.shape == (8, 125, 16, 4) and tsl3.shape == (8, 125, 3)
    assert np.array_equal(bits(quat3).reshape(1000, 16, 4), bits(quat)) and np.array_equal(bits(tsl3).reshape(1000, 3), bits(tsl))
    _, again = geometry.pose_repr_to_quat(pose)
    assert np.array_equal(bits(again), bits(quat))


# ---- outputs stay inside their buffers ----------------------------------------------------------------------------------------
def test_outputs_stay_inside_their_buffers():
    """every output carved out of a larger sentinel-filled tensor, at shapes off the tiles: the surroundings are untouched and every
    element inside is written (the entry points allocate nothing themselves)"""
    geometry = _geometry()
    # h2o / contact_min_dist: V = 257 and 1023, P = 257
    for i in (C.H2O_CASES.index((3, 5, 257, 3, 1, [2, 3, 1])), C.H2O_CASES.index((1, 5, 1023, 1, 257, None)),
              C.H2O_CASES.index((3, 2, 255, 3, 257, [3, 1, 2]))):
        B, T, V, nobj, P, _ = C.H2O_CASES[i]
        c = C.h2o_case(i)
        hv, tr, pts = c["hand"].cuda(), c["traj"].cuda(), c["pts"].cuda()
        on = None if c["obj_num"] is None else torch.tensor(c["obj_num"], dtype=torch.int32, device="cuda")
        for entry, n in (("tamf_h2o_dist", B * T * V), ("tamf_contact_min_dist", B * T)):
            big, out = _carved(n)
            rc, msg = _raw(entry, hv, tr, pts, on, B, T, V, nobj, P, out)
            assert rc == 0, msg
            _untouched_and_full(big, n)
            want = c["ref"] if n == B * T * V else c["ref"].min(dim=-1).values
            assert float((out.cpu().double().reshape(want.shape) - want).abs().max()) <= GATE_FACTOR * c["e32"]
    # pose decode: N J = 257 and 257 x 21
    for i in (C.POSE_CASES.index((257, 1)), C.POSE_CASES.index((257, 21))):
        c = C.pose_case(i)
        N, J = c["N"], c["J"]
        big_t, tsl = _carved(N * 3)
        big_q, quat = _carved(N * J * 4)
        rc, msg = _raw("tamf_pose_decode", c["pose"].cuda(), N, J, tsl, quat)
        assert rc == 0, msg
        _untouched_and_full(big_t, N * 3)
        _untouched_and_full(big_q, N * J * 4)
        assert float(C.quat_err(quat.cpu().numpy().reshape(N, J, 4), c["quat"]).max()) <= GATE_FACTOR * C.pose_gate_e32(i)
        big_q, quat = _carved(N * J * 4)  # without the translation output
        rc, msg = _raw("tamf_pose_decode", c["pose"].cuda(), N, J, None, quat)
        assert rc == 0, msg
        _untouched_and_full(big_q, N * J * 4)
    # transform_points, both types: P = 257 and 255 over (2, 3) objects x 3 frames
    for P in (257, 255):
        traj, pts, ref = C.transform_case(P)["calls"][-1]
        for dtype in (torch.float32, torch.float64):
            n = ref.numel()
            big, out = _carved(n, dtype)
            rc, msg = _raw("tamf_transform_points", traj.to(dtype).cuda(), pts.to(dtype).cuda(), 6, 3, P, int(dtype == torch.float64), out)
            assert rc == 0, msg
            _untouched_and_full(big, n)
            assert float((out.cpu().double().reshape(ref.shape) - ref).abs().max()) <= GATE_FACTOR * C.transform_case(P)["e32"]
    # vertex normals: n_mesh V = 2 x 257, 331 x 255, 1 x 3
    for V, M in ((257, 2), (255, 331), (3, 1)):
        c = C.normals_case(V, M)
        off, ent = geometry.vertex_incidence_csr(c["faces"], V)
        big, out = _carved(M * V * 3)
        rc, msg = _raw("tamf_vertex_normals", torch.from_numpy(c["verts"]).cuda(), M, V, torch.from_numpy(off).cuda(),
                       torch.from_numpy(ent).cuda(), out)
        assert rc == 0, msg
        _untouched_and_full(big, M * V * 3)  # (an unreferenced vertex is written too: 0, not the sentinel)
        assert float(np.abs(out.cpu().numpy().reshape(M, V, 3) - c["ref32"]).max()) <= 2e-7


# ---- refused arguments launch nothing -----------------------------------------------------------------------------------------
def _h2o_args(B, T, V, nobj, P):
    """tensors as large as the shape asks for (absolute values), so that a call that were not refused would stay inside them"""
    B_, T_, V_, o_, P_ = (max(1, abs(x)) for x in (B, T, V, nobj, P))
    g = torch.Generator().manual_seed(7)
    hv = (torch.randn(B_, T_, V_, 3, generator=g) * 0.1).cuda()
    tr = torch.randn(B_, o_, T_, 9, generator=g).cuda()
    pts = (torch.randn(B_, o_, P_, 3, generator=g) * 0.1).cuda()
    return hv, tr, pts, B_ * T_ * V_


def _refused(entry, args, out_big, text):
    rc, msg = _raw(entry, *args)
    assert rc == INVALID and text in msg, (entry, rc, msg)
    assert bool((out_big == SENTINEL).all()), entry  # nothing was launched


def test_h2o_refuses_what_it_cannot_run():
    for entry in ("tamf_h2o_dist", "tamf_contact_min_dist"):
        for shape, text in (((1, 1, 1025, 1, 1), "at most 1024 hand vertices"), ((65536, 1, 1, 1, 1), "batch too large"),
                            ((0, 1, 1, 1, 1), "bad shape"), ((1, 0, 1, 1, 1), "bad shape"), ((1, 1, 0, 1, 1), "bad shape"),
                            ((1, 1, 1, 0, 1), "bad shape"), ((1, 1, 1, 1, 0), "bad shape"), ((-1, 1, 1, 1, 1), "bad shape"),
                            ((1, -2, 1, 1, 1), "bad shape"), ((1, 1, -3, 1, 1), "bad shape"), ((1, 1, 1, -1, 1), "bad shape"),
                            ((1, 1, 1, 1, -256), "bad shape")):
            hv, tr, pts, n = _h2o_args(*shape)
            big, out = _carved(n)
            _refused(entry, (hv, tr, pts, None) + shape + (out,), big, text)
        hv, tr, pts, n = _h2o_args(2, 2, 5, 1, 3)
        big, out = _carved(n)
        for k in range(3):  # a null input; then the null output
            a = [hv, tr, pts]
            a[k] = None
            _refused(entry, tuple(a) + (None, 2, 2, 5, 1, 3, out), big, "null argument")
        _refused(entry, (hv, tr, pts, None, 2, 2, 5, 1, 3, None), big, "null argument")


def test_h2o_accepts_the_largest_batch_and_vertex_count():
    """B = 65535 (the grid's y limit) at T = V = P = 1, against the definition in float64; V = 1024 is in the parity table"""
    geometry = _geometry()
    B = 65535
    g = torch.Generator().manual_seed(11)
    hv = torch.randn(B, 1, 1, 3, generator=g) * 0.1
    tr = torch.randn(B, 1, 1, 9, generator=g)
    tr[..., 0:3] *= 0.05
    # of 65535 random rot6d some are ill-conditioned (a short vector, two nearly parallel ones) and would set e32 alone: the identity there
    a1, a2 = tr[..., 3:6], tr[..., 6:9]
    cos = (a1 * a2).sum(-1) / (a1.norm(dim=-1) * a2.norm(dim=-1))
    tr[(a1.norm(dim=-1) < 0.5) | (a2.norm(dim=-1) < 0.5) | (cos.abs() > 0.9)] = torch.tensor(C.IDENTITY_TRAJ)
    pts = torch.randn(B, 1, 1, 3, generator=g) * 0.1

    def definition(hv, tr, pts):
        R = G.rot6d_to_rotmat(tr[:, 0, 0, 3:9])
        return (hv[:, 0, 0] - (torch.einsum("bij,bj->bi", R, pts[:, 0, 0]) + tr[:, 0, 0, 0:3])).norm(dim=-1)

    ref = definition(hv.double(), tr.double(), pts.double())
    e32 = float((definition(hv, tr, pts).double() - ref).abs().max())
    got = geometry.multi_object_h2o_dist(hv.cuda(), tr.cuda(), pts.cuda())
    fmin = geometry.contact_min_dist(hv.cuda(), tr.cuda(), pts.cuda())
    err = float((got.cpu().double().reshape(B) - ref).abs().max())
    print(f"h2o B65535: HIP {err:.3e}, CPU float32 e32 {e32:.3e}, gate {GATE_FACTOR * e32:.3e}")
    assert 0 < e32 and err <= GATE_FACTOR * e32 and np.array_equal(bits(fmin).reshape(B), bits(got).reshape(B))
    assert any(c[2] == 1024 for c in C.H2O_CASES)


def test_the_other_entry_points_refuse_what_they_cannot_run():
    g = torch.Generator().manual_seed(13)
    # transform_points: n_obj = 65536 (above the grid's y limit), a zero dimension, a null pointer - in both types
    for is64, dtype in ((0, torch.float32), (1, torch.float64)):
        for (n_obj, T, P) in ((65536, 1, 1), (0, 2, 3), (2, 0, 3), (2, 2, 0), (-1, 2, 3)):
            no, t, p = max(1, abs(n_obj)), max(1, T), max(1, P)
            traj, pts = torch.randn(no, t, 9, generator=g).to(dtype).cuda(), torch.randn(no, p, 3, generator=g).to(dtype).cuda()
            big, out = _carved(no * t * p * 3, dtype)
            _refused("tamf_transform_points", (traj, pts, n_obj, T, P, is64, out), big, "bad shape")
        traj, pts = torch.randn(2, 2, 9, generator=g).to(dtype).cuda(), torch.randn(2, 3, 3, generator=g).to(dtype).cuda()
        big, out = _carved(36, dtype)
        for a in ((None, pts, 2, 2, 3, is64, out), (traj, None, 2, 2, 3, is64, out), (traj, pts, 2, 2, 3, is64, None)):
            _refused("tamf_transform_points", a, big, "null argument")
    # pose decode
    pose = torch.randn(4, 15, generator=g).cuda()
    big, out = _carved(4 * 2 * 4)
    for a in ((pose, 0, 2, None, out), (pose, 4, 0, None, out), (pose, -4, 2, None, out), (pose, 4, -2, None, out), (None, 4, 2, None, out),
              (pose, 4, 2, None, None)):
        _refused("tamf_pose_decode", a, big, "bad argument")
    # vertex normals
    c = C.normals_case(4, 2)
    off, ent = _geometry().vertex_incidence_csr(c["faces"], 4)
    v, off, ent = torch.from_numpy(c["verts"]).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(ent).cuda()
    big, out = _carved(2 * 4 * 3)
    for a in ((v, 0, 4, off, ent, out), (v, 2, 0, off, ent, out), (v, -2, 4, off, ent, out), (v, 2, -4, off, ent, out)):
        _refused("tamf_vertex_normals", a, big, "bad shape")
    for a in ((None, 2, 4, off, ent, out), (v, 2, 4, None, ent, out), (v, 2, 4, off, None, out), (v, 2, 4, off, ent, None)):
        _refused("tamf_vertex_normals", a, big, "null argument")


def test_wrapper_refuses_object_counts_outside_the_object_axis():
    """obj_num[b] must be in [1, nobj]: above it the kernel would clamp silently, at 0 or below it would return 1.7e19 for the clip"""
    geometry = _geometry()
    c = C.h2o_case(C.H2O_CASES.index((3, 2, 255, 3, 257, [3, 1, 2])))
    hv, tr, pts = c["hand"].cuda(), c["traj"].cuda(), c["pts"].cuda()
    for fn in (geometry.multi_object_h2o_dist, geometry.contact_min_dist):
        for bad, clip in (([3, 4, 2], 1), ([0, 1, 2], 0), ([3, 1, -1], 2)):
            with pytest.raises(ValueError, match=rf"obj_num\[{clip}\] = {bad[clip]} of clip {clip} is outside \[1, nobj = 3\]"):
                fn(hv, tr, pts, bad)
        assert fn(hv, tr, pts, [3, 1, 2]).shape[0] == 3  # the bounds themselves are accepted (1 and nobj)
