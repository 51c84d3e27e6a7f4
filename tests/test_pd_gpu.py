"""metrics/pd.py on the GPU: a hand-made clip with known answers - a small sphere "hand" pushed a known depth into the axis-aligned box
fixture - against the analytic depth (1e-12 relative) and against the restatement; zero for a hand outside; an object without a mesh
is left out."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")) if p not in sys.path]

import meshdist_cases as C  # noqa: E402
import meshdist_restatement as MR  # noqa: E402

pytestmark = pytest.mark.gpu

R_HAND = 0.01
T0 = np.asarray([0.5, -0.25, 0.125])  # the box objects' translations: float32 numbers, identity rotation, so that the float32
T1 = np.asarray([0.5, 0.25, 0.125])   # inverse pose is exact and the analytic depth holds to float64 rounding
FAR = np.asarray([5.0, 5.0, 5.0])
LEN = 41  # frames 0, 20, 40
#           (hand, frame): (object pushed into, depth in metres) - nothing listed: the hand is far away
PUSH = {(0, 0): (0, 0.004), (0, 40): (0, 0.009), (1, 0): (0, 0.002), (1, 40): (1, 0.0065)}


def _clip():
    from oracle.fixtures import icosphere

    v, f = C.fixture_mesh("aabox")
    lo, hi = v.min(0), v.max(0)
    ico = icosphere(1)[0]
    hands = np.zeros((2, LEN, len(ico), 3), np.float32)
    hands[:] = (FAR + R_HAND * ico).astype(np.float32)
    for (h, fr), (obj, depth) in PUSH.items():
        centre = (T0, T1)[obj] + np.asarray([hi[0] + R_HAND - depth, (lo[1] + hi[1]) / 2, (lo[2] + hi[2]) / 2])  # through the +x wall
        hands[h, fr] = (centre + R_HAND * ico).astype(np.float32)
    traj = np.zeros((2, LEN, 9), np.float32)
    traj[:, :, 3] = traj[:, :, 7] = 1.0  # rot6d of the identity
    traj[0, :, :3], traj[1, :, :3] = T0, T1
    return v, f, lo, hi, hands, traj


def _analytic_cm(hand32, t, lo, hi):
    """depth of one hand in one box object, centimetres: the largest distance to the nearest wall among the vertices inside"""
    q = hand32.astype(np.float64) - t
    inside = ((q > lo) & (q < hi)).all(1)
    wall = np.minimum(q - lo, hi - q).min(1)
    return 100.0 * float(np.where(inside, wall, 0.0).max()), bool(inside.any())


def test_known_depths_two_objects():
    from oakink2_tamf_amd.meshdist import MeshSet
    from oakink2_tamf_amd.metrics import pd as PD

    v, f, lo, hi, hands, traj = _clip()
    ms = MeshSet([(v, f), (v, f)])
    depth, pen = PD.clip_pd(hands[0], hands[1], traj, ms, [0, 1], LEN)
    assert depth.shape == (2, 3) and pen.tolist() == [[True, False, True], [True, False, True]]
    for h in (0, 1):
        for s, fr in enumerate((0, 20, 40)):
            per_obj = [_analytic_cm(hands[h, fr], t, lo, hi) for t in (T0, T1)]
            want = max(d for d, _ in per_obj)
            print("pd", h, fr, depth[h, s], want)
            assert abs(depth[h, s] - want) <= 1e-12 * want and pen[h, s] == any(p for _, p in per_obj)
            if (h, fr) in PUSH:  # and the known push, to the float32 rounding of the hand's vertices
                assert abs(depth[h, s] - 100.0 * PUSH[(h, fr)][1]) < 1e-4
            else:
                assert depth[h, s] == 0.0
    # the same by the restatement, bit for bit (sqrt and the factor 100 are correctly rounded on both sides)
    for h in (0, 1):
        for s, fr in enumerate((0, 20, 40)):
            best = 0.0
            for t in (T0, T1):
                q = MR.query_points(hands[h, fr], np.concatenate([np.eye(3), -t[:, None]], axis=1))
                d = MR.mesh_distance(v, f, q)[0]
                inside = ((q > lo) & (q < hi)).all(1)
                best = max(best, float(np.where(inside, d, 0.0).max()))
            assert depth[h, s] == best * 100.0
    # every other frame of the hand: stride 1 scores them all, the far hand gives 0
    d1, p1 = PD.clip_pd(hands[0], hands[1], traj, ms, [0, 1], LEN, stride=1)
    assert d1.shape == (2, LEN) and np.array_equal(d1[:, [0, 20, 40]], depth) and np.count_nonzero(d1) == 4 and p1.sum() == 4
    # culling changes nothing
    d2, p2 = PD.clip_pd(hands[0], hands[1], traj, ms, [0, 1], LEN, cull=False)
    assert np.array_equal(d2, depth) and np.array_equal(p2, pen)


def test_object_without_a_mesh_is_left_out():
    from oakink2_tamf_amd.meshdist import MeshSet
    from oakink2_tamf_amd.metrics import pd as PD

    v, f, lo, hi, hands, traj = _clip()
    ms = MeshSet([(v, f)])
    full, _ = PD.clip_pd(hands[0], hands[1], traj, MeshSet([(v, f), (v, f)]), [0, 1], LEN)
    depth, pen = PD.clip_pd(hands[0], hands[1], traj, ms, [0, None], LEN)  # object 1 has no mesh
    assert np.array_equal(depth[0], full[0]) and depth[1].tolist() == [full[1, 0], 0.0, 0.0] and pen[1].tolist() == [True, False, False]
    depth, pen = PD.clip_pd(hands[0], hands[1], traj, ms, [None, 0], LEN)  # object 0 has none: object 1 is mesh 0 of the set
    assert depth[0].tolist() == [0.0, 0.0, 0.0] and depth[1].tolist() == [0.0, 0.0, full[1, 2]]


def test_rotated_pose_against_the_restatement():
    """a general pose: the float32 inverse is no longer exact, so the yardstick is the restatement on the query points the host gives"""
    from oakink2_tamf_amd.meshdist import MeshSet
    from oakink2_tamf_amd.metrics import pd as PD
    from oakink2_tamf_amd.metrics import siv
    import torch

    from oakink2_tamf_amd.geometry import mesh_contains

    v, f = C.fixture_mesh("twoparts")
    rng = np.random.default_rng(4)
    traj = rng.normal(size=(1, 21, 9)).astype(np.float32)
    traj[..., :3] *= 0.1
    tf = siv.tslrot6d_to_transf(traj)
    local = C.points_around(v, 100, 9, expand=0.9)  # many of them inside
    hands = np.stack([(np.einsum("ij,pj->pi", tf[0, fr, :3, :3], local) + tf[0, fr, :3, 3]).astype(np.float32) for fr in range(21)])
    depth, pen = PD.clip_pd(hands, hands[::-1].copy(), traj, MeshSet([(v, f)]), [0], 21)
    inv = PD.inverse_transf(tf).astype(np.float64)
    for h, hv in enumerate((hands, hands[::-1])):
        for s, fr in enumerate((0, 20)):
            q = MR.query_points(hv[fr], inv[0, fr])
            d = MR.mesh_distance(v, f, q)[0]
            inside = mesh_contains(v, f, torch.from_numpy(q).cuda()).cpu().numpy()
            assert depth[h, s] == 100.0 * float(np.where(inside, d, 0.0).max()) and pen[h, s] == bool(inside.any())
    assert pen[0, 0] and depth[0, 0] > 0.0
