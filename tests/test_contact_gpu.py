"""GPU: the contact-distance kernels (libtamf_contact.so through oakink2_tamf_amd/contact.py) against the float64 torch restatement
tests/contact_restatement.py on the same float32 inputs.

Shapes: the smallest at which the kernels can go wrong - one vertex / point, one below, at and above the tile of 256, the MANO
hand's 778, the largest accepted V, a P that ends inside a tile; one and several frames, clips and objects, with ragged object counts.
Inputs: seeded clouds that are re-seeded, deterministically, until no decision sits where float32 rounding could flip it: relative gap
between nearest and second-nearest squared distance >= 1e-5 in both directions and |cos(n, y - x_near)| >= 1e-4, checked in float64.
With that, indices and signs must be EQUAL.  Distances and gradients: measured, not chosen - within 4 x the deviation of the float32
torch restatement from the float64 one on the same inputs (one figure per case: the largest deviation over all distances, or over
the gradient, relative to the largest float64 magnitude)."""
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import contact_restatement as CS  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VS, PS = (1, 255, 256, 257, 778, 1024), (1, 255, 256, 257, 600)
BIG, ONE = (3, 2, 3), (1, 1, 1)  # (T, B, nobj)
SWEEP = [(V, P) + BIG for V in VS for P in PS] + [(778, 257) + ONE, (1024, 600) + ONE, (778, 257, 1, 2, 3), (778, 257, 3, 1, 1)]
CORNERS = [(1, 1) + BIG, (1, 600) + BIG, (1024, 1) + BIG, (1024, 600) + BIG, (778, 257) + ONE, (257, 256) + BIG, (2, 600) + BIG]
_CASES = {}


def obj_num_of(B, nobj):
    return None if nobj == 1 else [nobj if b % 2 == 0 else 1 for b in range(B)]  # ragged: all, one, all, ...


def clouds(V, P, T, B, nobj, seed):
    g = torch.Generator().manual_seed(seed)
    hv = 0.1 * torch.randn(B, T, V, 3, generator=g)
    nrm = CS.unit(torch.randn(B, T, V, 3, generator=g))
    tr = torch.cat([0.05 * torch.randn(B, nobj, T, 3, generator=g), torch.randn(B, nobj, T, 6, generator=g)], dim=-1)
    pts = 0.1 * torch.randn(B, nobj, P, 3, generator=g)
    return tuple(t.to(DEV) for t in (hv, nrm, tr, pts))


def case(V, P, T, B, nobj):
    """inputs that meet the conditions, with the float64 and float32 restatements' results and the HIP results - computed once"""
    from oakink2_tamf_amd import contact

    key = (V, P, T, B, nobj)
    if key not in _CASES:
        on = obj_num_of(B, nobj)
        for seed in range(1000):
            inp = clouds(V, P, T, B, nobj, 1000 * (V + P) + seed)
            gap, cos = CS.conditions(*(t.double() for t in inp), on)
            if gap >= 1e-5 and cos >= 1e-4:
                break
        else:
            raise AssertionError("no seed met the conditions")
        r64 = CS.contact_all(*(t.double() for t in inp), on)
        r32 = CS.contact_all(*inp, on)
        hv, nrm, tr, pts = inp
        ont = None if on is None else torch.tensor(on, dtype=torch.int32, device=DEV)
        h2o, h2o_idx, o2h, o2h_idx = contact.contact_forward_raw(hv, nrm, tr, pts, ont)
        _CASES[key] = dict(inp=inp, on=on, ont=ont, r64=r64, r32=r32, hip=(o2h, h2o, o2h_idx, h2o_idx), seed=seed)
    return _CASES[key]


def deviation(got, want):
    """the largest deviation over the tensors of `got` from those of `want`, relative to the largest magnitude in `want`"""
    err = max(float((g.double() - w).abs().max()) for g, w in zip(got, want))
    return err / max(float(w.abs().max()) for w in want)


@pytest.mark.parametrize("V,P,T,B,nobj", SWEEP, ids=lambda v: str(v))
def test_forward_shape_sweep(V, P, T, B, nobj):
    c = case(V, P, T, B, nobj)
    o2h, h2o, o2h_idx, h2o_idx = c["hip"]
    r_o2h, r_h2o, r_o2h_idx, r_h2o_idx = c["r64"]
    assert h2o.shape == (B, nobj, T, V) and o2h.shape == (B, nobj, T, P) and h2o_idx.dtype == o2h_idx.dtype == torch.int32
    assert torch.equal(h2o_idx, r_h2o_idx) and torch.equal(o2h_idx, r_o2h_idx)
    assert torch.equal(o2h.sign().double(), r_o2h.sign()) and bool((h2o >= 0).all())
    hip_dev, ref_dev = deviation((h2o, o2h), (r_h2o, r_o2h)), deviation((c["r32"][1], c["r32"][0]), (r_h2o, r_o2h))
    print(f"CONTACT forward V={V} P={P} T={T} B={B} nobj={nobj} seed+{c['seed']}: hip {hip_dev:.3e}  float32 restatement {ref_dev:.3e}  gate {4 * ref_dev:.3e}")
    assert ref_dev > 0 and hip_dev <= 4 * ref_dev
    if c["on"] is not None:
        for b, n in enumerate(c["on"]):
            assert float(h2o[b, n:].abs().max() if n < nobj else 0) == 0 and float(o2h[b, n:].abs().max() if n < nobj else 0) == 0
            assert bool((h2o_idx[b, n:] == -1).all()) and bool((o2h_idx[b, n:] == -1).all())
            assert int(h2o_idx[b, :n].min()) >= 0 and int(o2h_idx[b, :n].min()) >= 0
    assert int(h2o_idx.max()) < P and int(o2h_idx.max()) < V


def test_directions_can_be_skipped_and_normals_left_out():
    from oakink2_tamf_amd import contact

    c = case(257, 256, *BIG)
    hv, nrm, tr, pts = c["inp"]
    o2h, h2o, o2h_idx, h2o_idx = c["hip"]
    a = contact.contact_forward_raw(hv, nrm, tr, pts, c["ont"], want_o2h=False)
    b = contact.contact_forward_raw(hv, nrm, tr, pts, c["ont"], want_h2o=False)
    assert a[2] is None and a[3] is None and torch.equal(a[0], h2o) and torch.equal(a[1], h2o_idx)
    assert b[0] is None and b[1] is None and torch.equal(b[2], o2h) and torch.equal(b[3], o2h_idx)
    u = contact.contact_forward_raw(hv, None, tr, pts, c["ont"])
    assert torch.equal(u[2], o2h.abs()) and torch.equal(u[3], o2h_idx) and bool((o2h < 0).any())
    # the public function: the same tensors, in point2point_signed's order
    p = contact.signed_contact_distance(hv, nrm, tr, pts, c["on"])
    assert torch.equal(p[0], o2h) and torch.equal(p[1], h2o) and torch.equal(p[2], o2h_idx)
    q = contact.signed_contact_distance(hv, nrm, tr, pts, c["on"], want_o2h=False)
    assert q[0] is None and q[2] is None and torch.equal(q[1], h2o)


IDENTITY = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def _exact(hand, normals, points):
    """one clip, one frame, one object in the identity pose, on small integer coordinates (exact in float32)"""
    from oakink2_tamf_amd import contact

    hv = torch.tensor(hand, dtype=torch.float32, device=DEV).reshape(1, 1, -1, 3).requires_grad_(True)
    nrm = None if normals is None else torch.tensor(normals, dtype=torch.float32, device=DEV).reshape(1, 1, -1, 3)
    pts = torch.tensor(points, dtype=torch.float32, device=DEV).reshape(1, 1, -1, 3)
    tr = torch.tensor(IDENTITY, dtype=torch.float32, device=DEV).reshape(1, 1, 1, 9)
    o2h, h2o, o2h_idx = contact.signed_contact_distance(hv, nrm, tr, pts)
    h2o_idx = contact.contact_forward_raw(hv.detach(), nrm, tr, pts, None)[1]
    return hv, o2h[0, 0, 0], h2o[0, 0, 0], o2h_idx[0, 0, 0], h2o_idx[0, 0, 0]


def test_exact_ties_take_the_lowest_index():
    hand = [[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0]]
    up = [[0, 0, 1]] * 4
    points = [[5, 5, 5], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [1, 1, 0], [1, 2, 3], [2, 1, -3]]
    _, o2h, h2o, o2h_idx, h2o_idx = _exact(hand, up, points)
    # vertex 0 is 1 away from points 1, 2 and 3
    assert int(h2o_idx[0]) == 1 and float(h2o[0].detach()) == 1.0
    # point 4 = (1,1,0) is sqrt(2) from all four vertices; point 5 is equally far from vertices 2 and 3; point 6 from 1 and 3
    assert o2h_idx.tolist()[4:] == [0, 2, 1]
    assert float(o2h[5]) == pytest.approx(10.0 ** 0.5, rel=1e-6) and float(o2h[6]) == pytest.approx(-(10.0 ** 0.5), rel=1e-6)
    # ties across tiles of 256 and across a thread's query slots: candidates 10 and 290, 5 and 260
    far = [[100 + i, 50, 50] for i in range(300)]
    pts = [list(p) for p in far]
    pts[10], pts[290] = [3, 0, 0], [0, 3, 0]
    _, _, h2o, _, h2o_idx = _exact([[0, 0, 0]], None, pts)
    assert int(h2o_idx[0]) == 10 and float(h2o[0]) == 3.0
    verts = [list(p) for p in far]
    verts[5], verts[260] = [0, 0, 4], [0, 4, 0]
    _, o2h, _, o2h_idx, _ = _exact(verts, None, [[0, 0, 0]])
    assert int(o2h_idx[0]) == 5 and float(o2h[0]) == 4.0
    _, _, _, o2h_idx, _ = _exact(list(reversed(verts)), None, [[0, 0, 0]])
    assert int(o2h_idx[0]) == 39  # (299 - 260: again the lower of the two)


def test_zero_signs_zero_distances_and_their_gradients():
    hand = [[0, 0, 0], [20, 0, 0], [0, 20, 0]]
    up = [[0, 0, 1]] * 3
    points = [[3, 4, 0], [20, 0, 0], [0, 0, 2], [1, 0, -2]]  # in vertex 0's tangent plane; on vertex 1; above and below vertex 0
    hv, o2h, h2o, o2h_idx, h2o_idx = _exact(hand, up, points)
    s5 = 5.0 ** 0.5
    assert o2h.tolist()[:3] == [0.0, 0.0, 2.0] and float(o2h[3]) == pytest.approx(-s5, rel=1e-6) and o2h_idx.tolist() == [0, 1, 0, 0]
    assert h2o_idx.tolist() == [2, 1, 0] and float(h2o[1]) == 0.0 and float(h2o[0]) == 2.0
    (o2h.sum() + h2o.sum()).backward()
    g = hv.grad[0, 0]
    assert torch.isfinite(g).all()
    # vertex 1: its own point coincides (zero, from both directions), nothing else is nearest to it
    assert g[1].tolist() == [0.0, 0.0, 0.0]
    # vertex 0: h2o towards point 2 gives (0,0,-1); o2h of point 0 has sign 0: nothing; of point 2: +1 * (0,0,-1); of point 3:
    # -1 * (x - y)/|x - y| = -(-1,0,2)/sqrt(5)
    want = torch.tensor([1.0 / s5, 0.0, -2.0 - 2.0 / s5])
    assert torch.allclose(g[0].cpu(), want, rtol=1e-6, atol=0)
    # unsigned without normals
    _, o2h_u, _, idx_u, _ = _exact(hand, None, points)
    assert o2h_u.tolist()[:3] == [5.0, 0.0, 2.0] and float(o2h_u[3]) == pytest.approx(s5, rel=1e-6) and idx_u.tolist() == [0, 1, 0, 0]


def _backward_case(V, P, T, B, nobj):
    """-> (hip gradient, float64 gradient, float32 restatement's gradient) of seeded upstream gradients"""
    from oakink2_tamf_amd import contact

    c = case(V, P, T, B, nobj)
    g = torch.Generator().manual_seed(V * 7 + P)
    up_o, up_h = torch.randn(B, nobj, T, P, generator=g).to(DEV), torch.randn(B, nobj, T, V, generator=g).to(DEV)
    grads = []
    for fn, dt in ((contact.signed_contact_distance, torch.float32), (CS.signed_contact_distance, torch.float64), (CS.signed_contact_distance, torch.float32)):
        hv, nrm, tr, pts = (t.detach().to(dt).clone() for t in c["inp"])
        hv.requires_grad_(True)
        if fn is contact.signed_contact_distance:
            tr.requires_grad_(True), pts.requires_grad_(True)
        o2h, h2o, o2h_idx = fn(hv, nrm, tr, pts, c["on"])
        assert not o2h_idx.requires_grad
        ((o2h * up_o.to(dt)).sum() + (h2o * up_h.to(dt)).sum()).backward()
        if fn is contact.signed_contact_distance:
            assert tr.grad is None and pts.grad is None and hv.grad.dtype == torch.float32  # the objects are data
        grads.append(hv.grad)
    return c, (up_o, up_h), grads


@pytest.mark.parametrize("V,P,T,B,nobj", CORNERS, ids=lambda v: str(v))
def test_backward_against_float64_autograd(V, P, T, B, nobj):
    c, _, (g_hip, g64, g32) = _backward_case(V, P, T, B, nobj)
    hip_dev, ref_dev = deviation((g_hip,), (g64,)), deviation((g32,), (g64,))
    print(f"CONTACT backward V={V} P={P} T={T} B={B} nobj={nobj}: hip {hip_dev:.3e}  float32 restatement {ref_dev:.3e}  gate {4 * ref_dev:.3e}")
    assert torch.isfinite(g_hip).all() and float(g64.abs().max()) > 0
    assert ref_dev > 0 and hip_dev <= 4 * ref_dev
    if V == 2:  # many points share one nearest vertex
        assert int(torch.bincount(c["hip"][2][c["hip"][2] >= 0].flatten().long()).max()) > 100


def test_backward_one_direction_at_a_time():
    from oakink2_tamf_amd import contact

    c, (up_o, up_h), (g_both, _, _) = _backward_case(257, 256, *BIG)
    hv, nrm, tr, pts = c["inp"]
    o2h, h2o, o2h_idx, h2o_idx = c["hip"]
    g_h = contact.contact_backward_raw(hv, tr, pts, c["ont"], h2o_idx, up_h, None, None, None)
    g_o = contact.contact_backward_raw(hv, tr, pts, c["ont"], None, None, o2h, o2h_idx, up_o)
    assert float(g_h.abs().max()) > 0 and float(g_o.abs().max()) > 0
    assert float((g_h + g_o - g_both).abs().max()) <= 1e-5 * float(g_both.abs().max())
    x = hv.clone().requires_grad_(True)
    _, h2o_only, _ = contact.signed_contact_distance(x, None, tr, pts, c["on"], want_o2h=False)
    (h2o_only * up_h).sum().backward()
    assert torch.equal(x.grad, g_h)
    with pytest.raises(RuntimeError, match="double backward"):
        x2 = hv.clone().requires_grad_(True)
        out = contact.signed_contact_distance(x2, nrm, tr, pts, c["on"])
        torch.autograd.grad(out[1].sum(), x2, create_graph=True)


def test_same_call_same_bits_and_a_clip_does_not_see_its_batch():
    from oakink2_tamf_amd import contact

    V, P, T, nobj = 778, 257, 3, 3
    hv, nrm, tr, pts = clouds(V, P, T, 3, nobj, 77)
    on = torch.tensor([3, 1, 2], dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(5)
    up_o, up_h = torch.randn(3, nobj, T, P, generator=g).to(DEV), torch.randn(3, nobj, T, V, generator=g).to(DEV)

    def run(sl):
        a = [t[sl].contiguous() for t in (hv, nrm, tr, pts)]
        h2o, h2o_idx, o2h, o2h_idx = contact.contact_forward_raw(*a, on[sl].contiguous())
        gh = contact.contact_backward_raw(a[0], a[2], a[3], on[sl].contiguous(), h2o_idx, up_h[sl].contiguous(), o2h, o2h_idx, up_o[sl].contiguous())
        return h2o, h2o_idx, o2h, o2h_idx, gh

    first, second = run(slice(0, 3)), run(slice(0, 3))
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    for b in range(3):
        alone = run(slice(b, b + 1))
        assert all(torch.equal(x[0], y[b]) for x, y in zip(alone, first)), b


def test_merged_h2o_dist_is_the_geometry_kernel_with_a_gradient():
    from oakink2_tamf_amd import contact, geometry

    c = case(778, 257, *BIG)
    hv, _, tr, pts = c["inp"]
    r_h2o = c["r64"][1]
    real = torch.tensor([[o < n for o in range(3)] for n in c["on"]], device=DEV)
    per_obj = torch.where(real[:, :, None, None], r_h2o, torch.full_like(r_h2o, float("inf")))
    two = torch.topk(per_obj, 2, dim=1, largest=False).values
    assert bool((two[:, 1] > two[:, 0]).all())  # no ties across objects
    x = hv.clone().requires_grad_(True)
    merged = contact.merged_h2o_dist(x, tr, pts, c["on"])
    assert torch.equal(merged, geometry.multi_object_h2o_dist(hv, tr, pts, c["on"]))
    up = torch.randn(merged.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    (merged * up).sum().backward()
    grads = []
    for dt in (torch.float64, torch.float32):
        y = hv.to(dt).requires_grad_(True)
        (CS.merged_h2o_dist(y, tr.to(dt), pts.to(dt), c["on"]) * up.to(dt)).sum().backward()
        grads.append(y.grad)
    hip_dev, ref_dev = deviation((x.grad,), (grads[0],)), deviation((grads[1],), (grads[0],))
    print(f"CONTACT merged gradient: hip {hip_dev:.3e}  float32 restatement {ref_dev:.3e}  gate {4 * ref_dev:.3e}")
    assert ref_dev > 0 and hip_dev <= 4 * ref_dev


def test_refusals_return_an_error_and_launch_nothing():
    """every call below is refused on the host before a launch; the buffers are nevertheless as large as the claimed shape needs"""
    from oakink2_tamf_amd import contact

    lib = contact._bind()
    INVALID = -1

    def buffers(B, T, V, nobj, P):
        f = lambda *s: torch.zeros(*[max(1, n) for n in s], device=DEV)  # noqa: E731
        i = lambda *s: torch.zeros(*[max(1, n) for n in s], device=DEV, dtype=torch.int32)  # noqa: E731
        return dict(hv=f(B, T, V, 3), nrm=f(B, T, V, 3), tr=f(B, nobj, T, 9), pts=f(B, nobj, P, 3), h2o=f(B, nobj, T, V), h2o_idx=i(B, nobj, T, V),
                    o2h=f(B, nobj, T, P), o2h_idx=i(B, nobj, T, P), g=f(B, T, V, 3))

    def fwd(dims, **null):
        t = {k: (None if k in null else v.data_ptr()) for k, v in buffers(*dims).items()}
        B, T, V, nobj, P = dims
        return lib.tamf_contact_forward(t["hv"], t["nrm"], t["tr"], t["pts"], None, B, T, V, nobj, P, t["h2o"], t["h2o_idx"], t["o2h"], t["o2h_idx"], None)

    def bwd(dims, **null):
        t = {k: (None if k in null else v.data_ptr()) for k, v in buffers(*dims).items()}
        B, T, V, nobj, P = dims
        return lib.tamf_contact_backward(t["hv"], t["tr"], t["pts"], None, B, T, V, nobj, P, t["h2o_idx"], t["h2o"], t["o2h"], t["o2h_idx"], t["o2h"],
                                         t["g"], None)

    def refused(rc, pattern):
        msg = lib.tamf_contact_last_error().decode()
        assert rc == INVALID and pattern in msg, (rc, msg)

    ok = (1, 1, 4, 1, 4)
    for call in (fwd, bwd):
        refused(call((1, 1, 1025, 1, 1)), "V outside [1, 1024]")
        refused(call((1, 1, 0, 1, 1)), "V outside [1, 1024]")
        for k in (0, 1, 3, 4):
            dims = list(ok)
            dims[k] = 0
            refused(call(tuple(dims)), "at least 1")
        refused(call((65536, 1, 1, 1, 1)), "B * nobj above 65535")
        refused(call(ok, hv=1), "null argument")
        refused(call(ok, tr=1), "null argument")
        refused(call(ok, pts=1), "null argument")
    refused(fwd(ok, h2o=1), "output pair")
    refused(fwd(ok, o2h_idx=1), "output pair")
    refused(fwd(ok, h2o=1, h2o_idx=1, o2h=1, o2h_idx=1), "nothing to compute")
    refused(bwd(ok, g=1), "null argument")
    refused(bwd(ok, h2o_idx=1), "g_h2o needs h2o_idx")
    refused(bwd(ok, o2h_idx=1), "g_o2h needs o2h_signed and o2h_idx")
    refused(bwd(ok, h2o=1, o2h=1), "no upstream gradient")
    assert fwd(ok) == 0 and bwd(ok) == 0  # and an accepted call goes through
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match=r"libtamf_contact: V outside \[1, 1024\]"):
        contact.signed_contact_distance(torch.zeros(1, 1, 1025, 3, device=DEV), None, torch.zeros(1, 1, 1, 9, device=DEV), torch.zeros(1, 1, 1, 3, device=DEV))
    with pytest.raises(ValueError, match="outside"):
        contact.signed_contact_distance(torch.zeros(1, 1, 4, 3, device=DEV), None, torch.zeros(1, 2, 1, 9, device=DEV), torch.zeros(1, 2, 1, 3, device=DEV), [3])
