"""GPU: the native point encoder (libtamf_pointenc.so, oakink2_tamf_amd.model.point_encoder.HipPointEncoder) against the reference's
PointTransformer as captured by tools/capture_pointenc_golden.py (tests/golden/pointenc_*.npz) on seeded weights
(tests/pointenc_fixture.py; regenerated here and checked against the fixture's checksum).

Tolerance: measured on the reference, never on the code under test.  e32 = max |float32 reference - float64 reference| on the case's
own inputs and groups, and the gate on the HIP output is 4 * e32 against the float64 output: both are fp32 evaluations of the same
sums in different orders, the factor covers the ordering difference, not more (the rule of tests/test_mano_gpu.py).

FPS: `tiny` and `mid` are captured under the condition that every iteration's two largest running minima are >= 1e-5 apart
(relative, in float32 and float64), so the exact sequence is tested.  A uniform 8192-point cloud does not meet that condition, so
`full` is tested on greedy validity, computed in float64 from the kernel's own sequence: each pick's running minimum is
>= (1 - 1e-5) x the largest running minimum at that step.  Neighbour sets are captured with a >= 1e-5 relative gap behind the last
member, so they are tested exactly, in all three cases."""
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
CASE_NAMES = ["tiny", "mid", "full"]
_CACHE = {}


def _case(name):
    """(fixture, state dict, encoder): built once per case and left unchanged"""
    if name not in _CACHE:
        from oakink2_tamf_amd.model.point_encoder import HipPointEncoder

        fix = load_golden(f"pointenc_{name}.npz")
        cfg = F.CASES[name][0]
        sd = F.seeded_state_dict(cfg, int(fix["weight_seed"]))
        assert F.state_checksum(sd) == str(fix["state_checksum"]), "the seeded weights are not the ones the fixture was captured with"
        enc = HipPointEncoder(cfg, device=DEV)
        enc.load_state_dict(sd)
        _CACHE[name] = (fix, sd, enc)
    return _CACHE[name]


@pytest.mark.parametrize("name", ["tiny", "mid"])
def test_fps_indices_equal_the_reference(name):
    fix, _, enc = _case(name)
    idx = enc.fps(fix["points"], start_index=fix["start"].astype(np.int64)).cpu().numpy()
    assert idx.dtype == np.int64 and np.array_equal(idx, fix["centre_idx"].astype(np.int64))


def test_fps_full_size_is_a_valid_greedy_sequence():
    fix, _, enc = _case("full")
    pts, start = fix["points"], fix["start"].astype(np.int64)
    idx = enc.fps(pts, start_index=start).cpu().numpy()
    B, G = idx.shape
    assert G == 512 and np.array_equal(idx[:, 0], start)
    for b in range(B):
        xyz = pts[b, :, :3].astype(np.float64)
        d = np.full(xyz.shape[0], np.inf)
        worst = np.inf
        for i in range(G - 1):
            d = np.minimum(d, ((xyz - xyz[idx[b, i]]) ** 2).sum(-1))
            worst = min(worst, d[idx[b, i + 1]] / d.max())
        print(f"full cloud {b}: min over steps of picked / largest running minimum = 1 - {1 - worst:.3e}")
        assert worst >= 1 - 1e-5 and len(set(idx[b].tolist())) == G


@pytest.mark.parametrize("name", CASE_NAMES)
def test_sorted_neighbour_sets_equal_the_reference(name):
    fix, _, enc = _case(name)
    pts = fix["points"]
    nbr = enc.group(pts, fix["centre_idx"].astype(np.int64)).cpu().numpy()
    assert np.array_equal(np.sort(nbr, -1), fix["nbr_sorted"].astype(np.int64))
    # ascending (distance, index) order, the centre itself first
    assert np.array_equal(nbr[..., 0], fix["centre_idx"].astype(np.int64))
    for b in range(pts.shape[0]):
        xyz = pts[b, :, :3].astype(np.float64)
        d = ((xyz[nbr[b]] - xyz[fix["centre_idx"][b].astype(np.int64)][:, None, :]) ** 2).sum(-1)
        assert (np.diff(d, axis=1) >= -1e-12).all()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_encode_parity_with_the_float64_reference(name):
    fix, _, enc = _case(name)
    out = enc.encode_groups(fix["points"], fix["centre_idx"].astype(np.int64), fix["nbr_sorted"].astype(np.int64)).cpu().numpy()
    assert out.shape == fix["out64"].shape and out.dtype == np.float32 and np.isfinite(out).all()
    err, e32 = float(np.abs(out.astype(np.float64) - fix["out64"]).max()), float(fix["e32"])
    print(f"{name}: max|hip - f64| = {err:.3e}, e32 = {e32:.3e}, ratio = {err / e32:.2f}")
    assert err <= 4 * e32


@pytest.mark.parametrize("name", ["tiny", "mid"])
def test_end_to_end_equals_the_staged_calls_bit_for_bit(name):
    fix, _, enc = _case(name)
    pts, start = torch.from_numpy(fix["points"]), fix["start"].astype(np.int64)
    centre = enc.fps(pts, start_index=start)
    staged = enc.encode_groups(pts, centre, enc.group(pts, centre))
    assert torch.equal(enc.encode(pts, start_index=start), staged)
    # a seed draws the start from a CPU generator; the default start is index 0
    g = torch.Generator().manual_seed(5)
    drawn = torch.randint(0, pts.shape[1], (pts.shape[0],), generator=g)
    assert torch.equal(enc.encode(pts, seed=5), enc.encode(pts, start_index=drawn))
    assert torch.equal(enc.encode(pts), enc.encode(pts, start_index=0))


@pytest.mark.parametrize("name", ["tiny", "mid"])
def test_a_cloud_alone_and_in_a_batch_of_three_gives_the_same_bits(name):
    fix, _, enc = _case(name)
    pts = torch.from_numpy(fix["points"])
    other = torch.from_numpy(F.seeded_clouds(2, pts.shape[1], pts.shape[2], 7))
    alone = enc.encode(pts[1:2], start_index=3)
    for pos in range(3):
        batch = torch.cat([other[:pos], pts[1:2], other[pos:]], 0)
        assert batch.shape[0] == 3 and torch.equal(enc.encode(batch, start_index=3)[pos:pos + 1], alone)


def test_fps_above_the_register_variants():
    """N = 9000 (16 points per thread in registers) and N = 20000 (coordinates re-read through L2) against a float32 numpy FPS of
    the same expression; on these seeded clouds the two largest running minima stay >= 1e-5 apart (asserted), so the sequence is exact"""
    from oakink2_tamf_amd.model.point_encoder import HipPointEncoder

    enc = HipPointEncoder(F.CASES["tiny"][0], device=DEV)
    rng = np.random.default_rng(3)
    for N, G in ((20000, 40), (9000, 40)):
        xyz = rng.uniform(-1, 1, (1, N, 3)).astype(np.float32)
        want, gap = F.host_fps(xyz[0], G, N - 1)
        assert gap >= 1e-5
        assert enc.fps(xyz, num=G, start_index=N - 1).cpu().numpy()[0].tolist() == want.tolist()


def test_errors():
    from oakink2_tamf_amd.model.point_encoder import HipPointEncoder, PointEncoderError

    fix, sd, enc = _case("tiny")
    cfg = F.CASES["tiny"][0]
    missing = {k: v for k, v in sd.items() if k != "blocks.blocks.1.attn.proj.bias"}
    with pytest.raises(PointEncoderError, match="missing key 'blocks.blocks.1.attn.proj.bias'"):
        HipPointEncoder(cfg, device=DEV).load_state_dict(missing)
    wrong = dict(sd)
    wrong["reduce_dim.weight"] = sd["reduce_dim.weight"][:, :-1]
    with pytest.raises(PointEncoderError, match="reduce_dim.weight: expected shape"):
        HipPointEncoder(cfg, device=DEV).load_state_dict(wrong)
    bad = dict(sd)
    bad["norm.bias"] = sd["norm.bias"].copy()
    bad["norm.bias"][3] = np.inf
    with pytest.raises(PointEncoderError, match="norm.bias: holds a non-finite value"):
        HipPointEncoder(cfg, device=DEV).load_state_dict(bad)
    pts = fix["points"].copy()
    pts[1, 7, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        enc.encode(pts)
    with pytest.raises(ValueError, match="non-finite"):
        enc.fps(pts)
    with pytest.raises(PointEncoderError, match="no weights loaded"):
        HipPointEncoder(cfg, device=DEV).encode(fix["points"])
    with pytest.raises(ValueError, match="outside"):
        enc.encode_groups(fix["points"], fix["centre_idx"].astype(np.int64) + 250, fix["nbr_sorted"].astype(np.int64))
    with pytest.raises(PointEncoderError, match="group_size"):
        HipPointEncoder(dict(cfg, group_size=4), device=DEV)
