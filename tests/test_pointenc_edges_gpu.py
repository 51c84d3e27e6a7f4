"""GPU: the native point encoder (libtamf_pointenc.so) across the shape ranges tamf_pointenc_model_create accepts, not only at the
three configurations of tests/test_pointenc_gpu.py.  References: tests/pointenc_fixture.restatement in float64 (pinned to the
reference's captured outputs by tests/test_pointenc_cpu.py) for the encoder, and the float32 host emulations host_fps / host_knn of
include/tamf_pointenc.h's selection rules for FPS and grouping.

Encoder tolerance: the project's rule, unchanged (tests/test_pointenc_gpu.py, tests/test_mano_gpu.py): e32 = max |float32 restatement
- float64 restatement| on the case's own inputs, computed on the CPU; the gate on the HIP output is 4 * e32 against the float64
restatement.  FPS and grouping are compared exactly: both sides evaluate ((dx*dx + dy*dy) + dz*dz) in float32 with every operation
rounded on its own, and the header fixes the order among equals, so no near-tie condition is needed.

What the SWEEP cases of tests/pointenc_fixture.py reach (T = num_group + 1 tokens, Tp = round_up(T, 4)):
  attn_kernel   T = 2, 16 (one full query panel), 17 (a panel with one live row); Tp - T = 0, 1, 2, 3; Tp % 8 == 0 (no odd tail step
                of the P.V loop); T = 992 / 993 on either side of 64 KiB of dynamic LDS (hipFuncSetAttribute), T = 1025
  gemm_kernel   encoder_dims 16, 48, 80 (column tail, K tail of reduce_dim), 1024; trans_dim 1024 (3072 / 4096 columns, 16 heads);
                group_size 9, 33, 63, 64 (radd row grouping, row tails)
  encode_groups batches of 5 and 9 clouds: calls of 4 + 1 and 4 + 4 + 1 on one workspace, batch invariance across the chunk edges
  fps_kernel    N = 1, 40, 63 (waves without a point), 8192 / 8193 and 16384 / 16385 (the three variants), 32768; G = N; exact ties
  group_kernel  M = N, N not a multiple of 256, N = 16384 / 16385 (64 KiB of LDS), 32768; exact ties
  C interface   outputs and an exactly sized workspace carved out of sentinel-filled tensors; every refusal of the header

Measured err / e32 ratios (gate 4): none recorded yet - when this file was written it had been collected and its references run on
the CPU, but it had not run on an MI355X.  Every encoder test prints its err, e32 and ratio; record them here from the first run."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import pointenc_fixture as F  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_MAX = 32768
SENT_I, SENT_F = -7, -12345.0  # no index is negative; outputs stay below |4| (LayerNorm of seeded weights)
_ENC = {}


def _plain():
    """an encoder without weights: fps and group do not use the model"""
    if "plain" not in _ENC:
        from oakink2_tamf_amd.model.point_encoder import HipPointEncoder

        _ENC["plain"] = HipPointEncoder(F.CASES["tiny"][0], device=DEV)
    return _ENC["plain"]


def _sweep(name):
    """(case, encoder): built once per case and left unchanged"""
    if name not in _ENC:
        from oakink2_tamf_amd.model.point_encoder import HipPointEncoder

        c = F.sweep_case(name)
        enc = HipPointEncoder(c["cfg"], device=DEV)
        enc.load_state_dict(c["sd"])
        _ENC[name] = (c, enc)
    return _ENC[name]


def _gate(tag, out, out64, e32):
    err = float(np.abs(out.astype(np.float64) - out64).max())
    print(f"{tag}: max|hip - f64| = {err:.3e}, e32 = {e32:.3e}, ratio = {err / e32:.2f}")
    assert e32 > 0
    assert err <= 4 * e32


# ---- the encoder across the accepted configurations ----
@pytest.mark.parametrize("name", list(F.SWEEP))
def test_encode_sweep_parity_with_the_float64_restatement(name):
    c, enc = _sweep(name)
    out = enc.encode_groups(c["points"], c["centre_idx"], c["nbr_idx"]).cpu().numpy()
    assert out.shape == (F.SWEEP[name][2], 2 * c["cfg"]["trans_dim"]) and out.dtype == np.float32 and np.isfinite(out).all()
    _gate(name, out, c["out64"], c["e32"])


def test_batch_of_nine_is_cut_into_calls_of_four_four_and_one():
    """`tiny` with B = 9: one cloud alone gives the same bits as that cloud at positions 3 (last of the first call), 4 (first of
    the second) and 8 (the call of one); the whole batch meets the gate"""
    from oakink2_tamf_amd.model.point_encoder import MAX_CLOUDS_PER_CALL, HipPointEncoder

    assert MAX_CLOUDS_PER_CALL == 4
    cfg, N, _ = F.CASES["tiny"]
    sd = F.seeded_state_dict(cfg, F.WEIGHT_SEED["tiny"])
    assert F.state_checksum(sd) == str(load_golden("pointenc_tiny.npz")["state_checksum"])
    enc = HipPointEncoder(cfg, device=DEV)
    enc.load_state_dict(sd)
    pts = F.seeded_clouds(10, N, cfg["point_dims"], 31)
    ci, ni = F.drawn_groups(pts, cfg["num_group"], cfg["group_size"], 32)
    alone = enc.encode_groups(pts[9:], ci[9:], ni[9:])
    for pos in (3, 4, 8):
        sel = [i for i in range(9) if i != pos]
        sel.insert(pos, 9)
        batch = enc.encode_groups(pts[sel], ci[sel], ni[sel])
        assert batch.shape == (9, 2 * cfg["trans_dim"]) and torch.equal(batch[pos:pos + 1], alone), pos
    out64 = F.restatement(sd, cfg, pts[sel], ci[sel], ni[sel], torch.float64).numpy()
    out32 = F.restatement(sd, cfg, pts[sel], ci[sel], ni[sel], torch.float32).numpy()
    out = batch.cpu().numpy()
    assert np.isfinite(out).all()
    _gate("tiny x 9", out, out64, float(np.abs(out32.astype(np.float64) - out64).max()))


# ---- farthest-point sampling ----
def _fps_check(xyz, G, starts):
    """one cloud, one call with a batch entry per start index, against host_fps"""
    pts = np.repeat(xyz[None], len(starts), 0)
    got = _plain().fps(pts, num=G, start_index=np.asarray(starts, dtype=np.int64)).cpu().numpy()
    assert got.shape == (len(starts), G) and got.dtype == np.int64
    want = np.stack([F.host_fps(xyz, G, s)[0] for s in starts])
    assert np.array_equal(got, want), (xyz.shape, G, starts, np.argwhere(got != want)[:4].tolist())
    return want


@pytest.mark.parametrize("N,G", [(1, 1), (40, 8), (40, 40), (63, 8), (8192, 8), (8193, 8), (16384, 8), (16385, 8), (N_MAX, 8)])
def test_fps_equals_the_host_emulation(N, G):
    xyz = np.random.default_rng(1000 + N).uniform(-1, 1, (N, 3)).astype(np.float32)
    want = _fps_check(xyz, G, sorted({0, N // 2, N - 1}))
    assert all(len(set(r.tolist())) == G for r in want)  # (no duplicates among distinct points)


def test_fps_exact_tie_goes_to_the_lowest_index():
    """two points are mirror images about the start, farther out than everything else: the first pick is an exact tie.  2500
    points: the pair sits in different waves and different per-thread slots; 9000: the 16-points-per-thread variant."""
    for N, lo, hi, start in ((2500, 37, 2300, 1300), (9000, 8500, 8800, 3)):
        rng = np.random.default_rng(N)
        xyz = (np.array([0.5, 0.25, -0.125]) + rng.uniform(-0.5, 0.5, (N, 3))).astype(np.float32)
        xyz[start] = [0.5, 0.25, -0.125]
        xyz[lo], xyz[hi] = [2.5, 1.25, 0.375], [-1.5, -0.75, -0.625]  # start +- (2, 1, 0.5), exact in float32
        want = _fps_check(xyz, 6, [start])
        d = ((xyz - xyz[start]) ** 2).sum(-1)
        assert d[lo] == d[hi] == d.max() and want[0, 1] == lo


def test_fps_on_duplicate_points_until_the_minima_reach_zero():
    xyz = np.random.default_rng(9).uniform(-1, 1, (120, 3)).astype(np.float32)
    xyz[10:60] = xyz[10]
    want = _fps_check(xyz, 120, [0, 30, 119])
    assert len(set(want[0].tolist())) == 71 and (want[:, 71:] == 0).all()  # every distinct point once, then index 0 among all-zero minima


# ---- grouping ----
def _group_check(pts, centre, M):
    got = _plain().group(pts, centre, group_size=M).cpu().numpy()
    want = np.stack([F.host_knn(pts[b], centre[b], M) for b in range(pts.shape[0])])
    assert got.shape == want.shape and got.dtype == np.int64
    assert np.array_equal(got, want), (pts.shape, M, np.argwhere(got != want)[:4].tolist())
    return want


@pytest.mark.parametrize("N,M", [(8, 8), (300, 300), (1000, 9), (16384, 8), (16385, 8), (N_MAX, 64)])
def test_group_equals_the_host_emulation(N, M):
    rng = np.random.default_rng(2000 + N)
    pts = rng.uniform(-1, 1, (2, N, 3)).astype(np.float32)
    centre = np.stack([rng.choice(N, 4, replace=False) for _ in range(2)])
    centre[1, 3] = N - 1
    want = _group_check(pts, centre, M)
    assert np.array_equal(want[..., 0], centre)
    if M == N:
        assert (np.sort(want, -1) == np.arange(N)).all()


def test_group_orders_exact_ties_by_index():
    """50 points are exact copies of 50 others and two centres lie among them (an original and a copy): equal distances come in
    pairs, an odd group size cuts a pair, and the centre itself is not the first of its pair when it is the copy"""
    rng = np.random.default_rng(13)
    pts = rng.uniform(-1, 1, (2, 300, 6)).astype(np.float32)
    pts[:, 200:250, :3] = pts[:, 100:150, :3]
    centre = np.array([[120, 220, 5, 299], [249, 100, 0, 150]])
    want = _group_check(pts, centre, 9)
    assert want[0, 0, :2].tolist() == [120, 220] and want[0, 1, :2].tolist() == [120, 220] and want[1, 0, :2].tolist() == [149, 249]


# ---- the C interface: guard tails and refusals ----
def _lib():
    from oakink2_tamf_amd.model.point_encoder import _bind

    return _bind()


def _stream():
    return int(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _carve(n, dtype, sentinel, pre=64, tail=1024):
    """(whole, region): `region` = n elements inside a larger sentinel-filled tensor, 256 bytes from its start"""
    whole = torch.full((pre + n + tail,), sentinel, dtype=dtype, device=DEV)
    return whole, whole[pre:pre + n]


def _untouched(whole, n, sentinel, pre=64):
    return bool((whole[:pre] == sentinel).all()) and bool((whole[pre + n:] == sentinel).all())


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def _raw_encode(enc, p, ci, ni, B, N, out, ws, nbytes, model=None):
    lib = _lib()
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())  # noqa: E731
    rc = lib.tamf_pointenc_encode(enc._model if model is None else model, ptr(p), ptr(ci), ptr(ni), B, N, ptr(out), ptr(ws), nbytes, _stream())
    torch.cuda.synchronize()
    return rc, lib.tamf_pointenc_last_error().decode()


@pytest.mark.parametrize("name", ["odd", "g1024"])
def test_c_calls_stay_inside_their_outputs_and_the_exact_workspace(name):
    c, enc = _sweep(name)
    lib, cfg = _lib(), c["cfg"]
    B, N, C = c["points"].shape
    G, M, D = cfg["num_group"], cfg["group_size"], cfg["trans_dim"]
    p = _dev(c["points"], torch.float32)
    ci, ni = _dev(c["centre_idx"], torch.int32), _dev(c["nbr_idx"], torch.int32)
    start = _dev(c["centre_idx"][:, 0], torch.int32)
    # fps
    whole, idx = _carve(B * G, torch.int32, SENT_I)
    assert lib.tamf_pointenc_fps(p.data_ptr(), start.data_ptr(), B, N, C, G, idx.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert _untouched(whole, B * G, SENT_I) and bool((idx != SENT_I).all())
    want = np.stack([F.host_fps(c["points"][b], G, int(c["centre_idx"][b, 0]))[0] for b in range(B)])
    assert np.array_equal(idx.cpu().numpy().reshape(B, G), want)
    # group
    whole, nbr = _carve(B * G * M, torch.int32, SENT_I)
    assert lib.tamf_pointenc_group(p.data_ptr(), ci.data_ptr(), B, N, C, G, M, nbr.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert _untouched(whole, B * G * M, SENT_I) and bool((nbr != SENT_I).all())
    assert np.array_equal(nbr.cpu().numpy().reshape(B, G, M), c["nbr_idx"])
    # encode: the workspace is exactly tamf_pointenc_workspace_bytes, then a tail (B <= 4 per call, as the wrapper calls it)
    want = enc.encode_groups(c["points"], c["centre_idx"], c["nbr_idx"])
    for b0 in range(0, B, 4):
        n = min(4, B - b0)
        nbytes = int(lib.tamf_pointenc_workspace_bytes(enc._model, n))
        assert nbytes > 0 and nbytes % 16 == 0
        wsw, ws = _carve(nbytes // 4, torch.float32, SENT_F)
        ow, out = _carve(n * 2 * D, torch.float32, SENT_F)
        assert ws.data_ptr() % 16 == 0
        rc, msg = _raw_encode(enc, p[b0:], ci[b0:], ni[b0:], n, N, out, ws, nbytes)
        assert rc == 0, msg
        assert _untouched(wsw, nbytes // 4, SENT_F) and _untouched(ow, n * 2 * D, SENT_F) and bool((out != SENT_F).all())
        assert torch.equal(out.reshape(n, 2 * D), want[b0:b0 + n])


def test_c_calls_refuse_bad_arguments_and_write_nothing():
    c, enc = _sweep("odd")
    lib, cfg = _lib(), c["cfg"]
    B, N, C = c["points"].shape
    G, M, D = cfg["num_group"], cfg["group_size"], cfg["trans_dim"]
    p = _dev(c["points"], torch.float32)
    ci, ni = _dev(c["centre_idx"], torch.int32), _dev(c["nbr_idx"], torch.int32)
    start = _dev(c["centre_idx"][:, 0], torch.int32)
    idx = torch.full((B * N,), SENT_I, dtype=torch.int32, device=DEV)
    nbr = torch.full((B * G * N,), SENT_I, dtype=torch.int32, device=DEV)
    out = torch.full((B * 2 * D,), SENT_F, dtype=torch.float32, device=DEV)
    nbytes = int(lib.tamf_pointenc_workspace_bytes(enc._model, B))
    ws = torch.full((nbytes // 4 + 4,), SENT_F, dtype=torch.float32, device=DEV)
    INVALID, STATE = -1, -2  # TAMF_ERR_INVALID, TAMF_ERR_STATE of include/tamf_hip.h

    def refused(rc, want, *words):
        msg = lib.tamf_pointenc_last_error().decode()
        assert rc == want and msg and all(w in msg for w in words), (rc, msg)

    s = _stream()
    P, S, I, CI, NB = p.data_ptr(), start.data_ptr(), idx.data_ptr(), ci.data_ptr(), nbr.data_ptr()
    for args in ((None, S, B, N, C, G, I, s), (P, None, B, N, C, G, I, s), (P, S, B, N, C, G, None, s)):
        refused(lib.tamf_pointenc_fps(*args), INVALID, "null")
    refused(lib.tamf_pointenc_fps(P, S, B, N, C, N + 1, I, s), INVALID, "G = %d" % (N + 1))
    refused(lib.tamf_pointenc_fps(P, S, B, N, C, 0, I, s), INVALID, "G = 0")
    refused(lib.tamf_pointenc_fps(P, S, B, N_MAX + 1, C, G, I, s), INVALID, "N = %d" % (N_MAX + 1))
    refused(lib.tamf_pointenc_fps(P, S, B, N, 2, G, I, s), INVALID, "C = 2")
    for args in ((None, CI, B, N, C, G, M, NB, s), (P, None, B, N, C, G, M, NB, s), (P, CI, B, N, C, G, M, None, s)):
        refused(lib.tamf_pointenc_group(*args), INVALID, "null")
    refused(lib.tamf_pointenc_group(P, CI, B, N, C, G, N + 1, NB, s), INVALID, "M = %d" % (N + 1))
    refused(lib.tamf_pointenc_group(P, CI, B, N_MAX + 1, C, G, M, NB, s), INVALID, "N = %d" % (N_MAX + 1))
    refused(lib.tamf_pointenc_group(P, CI, 0, N, C, G, M, NB, s), INVALID, "B = 0")

    def enc_refused(want, *words, **kw):
        a = dict(p=p, ci=ci, ni=ni, B=B, N=N, out=out, ws=ws, nbytes=nbytes, model=None)
        a.update(kw)
        rc, msg = _raw_encode(enc, **a)
        assert rc == want and msg and all(w in msg for w in words), (rc, msg)

    for k in ("p", "ci", "ni", "out", "ws"):
        enc_refused(INVALID, "null", **{k: None})
    rc = lib.tamf_pointenc_encode(None, P, CI, ni.data_ptr(), B, N, out.data_ptr(), ws.data_ptr(), nbytes, s)
    refused(rc, INVALID, "null")
    enc_refused(INVALID, "N = %d" % (N_MAX + 1), N=N_MAX + 1)
    enc_refused(INVALID, "group_size", N=M - 1)
    enc_refused(INVALID, "workspace of %d bytes, need %d" % (nbytes - 1, nbytes), nbytes=nbytes - 1)
    enc_refused(INVALID, "aligned", ws=ws.data_ptr() + 4)
    assert lib.tamf_pointenc_workspace_bytes(None, B) == 0 and lib.tamf_pointenc_workspace_bytes(enc._model, 0) == 0
    from oakink2_tamf_amd.model.point_encoder import HipPointEncoder

    empty = HipPointEncoder(cfg, device=DEV)  # created, nothing loaded, not finalised
    enc_refused(STATE, "not finalised", model=empty._model)
    torch.cuda.synchronize()
    assert bool((idx == SENT_I).all()) and bool((nbr == SENT_I).all()) and bool((out == SENT_F).all()) and bool((ws == SENT_F).all())


def test_an_index_outside_the_cloud_is_read_as_zero_and_stays_with_its_cloud():
    """the header's rule for the C calls (the Python wrapper refuses such indices before they get here): cloud 0 carries indices
    outside [0, N), cloud 1 does not - cloud 1's results keep their bits, cloud 0's are those of index 0 in their place"""
    c, enc = _sweep("odd")
    lib, cfg = _lib(), c["cfg"]
    B, N, C = 2, c["points"].shape[1], c["points"].shape[2]
    G, M, D = cfg["num_group"], cfg["group_size"], cfg["trans_dim"]
    pts, ci, ni = c["points"][:2], c["centre_idx"][:2].copy(), c["nbr_idx"][:2].copy()
    bad_ci, bad_ni = ci.copy(), ni.copy()
    bad_ci[0, 2], bad_ci[0, 7], bad_ni[0, 1, 3], bad_ni[0, 14, 8] = -1, N, N + 5, -(2 ** 31)
    ci[0, 2] = ci[0, 7] = ni[0, 1, 3] = ni[0, 14, 8] = 0
    want = enc.encode_groups(pts, ci, ni)
    nbytes = int(lib.tamf_pointenc_workspace_bytes(enc._model, B))
    wsw, ws = _carve(nbytes // 4, torch.float32, SENT_F)
    ow, out = _carve(B * 2 * D, torch.float32, SENT_F)
    rc, msg = _raw_encode(enc, _dev(pts, torch.float32), _dev(bad_ci, torch.int32), _dev(bad_ni, torch.int32), B, N, out, ws, nbytes)
    assert rc == 0, msg
    assert torch.equal(out.reshape(B, 2 * D), want) and _untouched(wsw, nbytes // 4, SENT_F) and _untouched(ow, B * 2 * D, SENT_F)
    # fps start and group centres
    p = _dev(pts, torch.float32)
    idx = torch.full((B, 6), SENT_I, dtype=torch.int32, device=DEV)
    assert lib.tamf_pointenc_fps(p.data_ptr(), _dev([N + 3, 5], torch.int32).data_ptr(), B, N, C, 6, idx.data_ptr(), _stream()) == 0
    nbr = torch.full((B, G, M), SENT_I, dtype=torch.int32, device=DEV)
    assert lib.tamf_pointenc_group(p.data_ptr(), _dev(bad_ci, torch.int32).data_ptr(), B, N, C, G, M, nbr.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), np.stack([F.host_fps(pts[0], 6, 0)[0], F.host_fps(pts[1], 6, 5)[0]]))
    assert np.array_equal(nbr.cpu().numpy(), np.stack([F.host_knn(pts[b], ci[b], M) for b in range(B)]))
