"""metrics/pd.py without a GPU: the job list, the inverse poses, the frame reduction and the units on hand-made distances, and
render.penetration_colors."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")) if p not in sys.path]

from oakink2_tamf_amd.metrics import pd as PD  # noqa: E402
from oakink2_tamf_amd.metrics import siv  # noqa: E402


def test_job_list_is_sivs_with_hand_slices():
    jobs = PD.clip_jobs(45, [3, None, 0], 778)
    sj = siv.clip_jobs(45, [10, None, 20])
    assert PD.STRIDE == siv.STRIDE == 20 and jobs["frames"].tolist() == [0, 20, 40]
    for key in ("frames", "frame_slot", "hand", "obj"):
        assert np.array_equal(jobs[key], sj[key]), key
    assert jobs["obj"].tolist() == [0, 2] * 6 and jobs["mesh_id"].tolist() == [3, 0] * 6 and jobs["mesh_id"].dtype == np.int32
    assert jobs["pt_off"].tolist() == [0, 0, 778, 778, 1556, 1556, 2334, 2334, 3112, 3112, 3890, 3890] and (jobs["pt_len"] == 778).all()
    assert PD.clip_jobs(45, [3], 778, stride=45)["frames"].tolist() == [0] and PD.clip_jobs(0, [3], 778)["frames"].size == 0
    assert PD.clip_jobs(45, [None, None], 778)["mesh_id"].size == 0


def test_inverse_transf_is_rt_and_minus_rt_t_in_the_input_dtype():
    rng = np.random.default_rng(0)
    traj = rng.normal(size=(2, 5, 9)).astype(np.float32)
    t = siv.tslrot6d_to_transf(traj)
    inv = PD.inverse_transf(t)
    assert inv.dtype == np.float32 and inv.shape == (2, 5, 3, 4)
    R, tt = t[..., :3, :3], t[..., :3, 3]
    assert np.array_equal(inv[..., :3], np.swapaxes(R, -1, -2))
    assert np.array_equal(inv[..., 3], -np.matmul(np.swapaxes(R, -1, -2), tt[..., None])[..., 0])
    # it undoes the pose to float32 accuracy
    p = rng.normal(size=(7, 3))
    world = np.einsum("...ij,pj->...pi", R.astype(np.float64), p) + tt[..., None, :]
    back = np.einsum("...ij,...pj->...pi", inv[..., :3].astype(np.float64), world) + inv[..., None, :, 3]
    assert np.abs(back - p).max() < 1e-5
    assert PD.inverse_transf(t.astype(np.float64)).dtype == np.float64


def test_frame_reduction_and_units_on_hand_made_distances():
    V = 4
    jobs = PD.clip_jobs(41, [0, 1], V)  # frames 0, 20, 40; per frame: gt x (obj 0, obj 1), refined x (obj 0, obj 1)
    J = len(jobs["mesh_id"])
    assert J == 12
    dist = np.full((J, V), 0.5)  # metres; far values that must not count where the vertex is outside
    inside = np.zeros((J, V), bool)
    dist[0] = [0.001, 0.004, 0.5, 0.5]; inside[0] = [1, 1, 0, 0]      # frame 0, gt, obj 0: 4 mm
    dist[1] = [0.5, 0.5, 0.5, 0.0125]; inside[1] = [0, 0, 0, 1]       # frame 0, gt, obj 1: 12.5 mm -> the frame's depth
    dist[2] = [0.002, 0.5, 0.5, 0.5]; inside[2] = [1, 0, 0, 0]        # frame 0, refined, obj 0: 2 mm
    dist[6] = [0.0, 0.5, 0.5, 0.5]; inside[6] = [1, 0, 0, 0]          # frame 20, refined, obj 0: inside at depth exactly 0
    dist[9] = [0.5, 0.03, 0.5, 0.5]; inside[9] = [0, 1, 0, 0]         # frame 40, gt, obj 1: 3 cm
    depth, pen = PD.reduce_frames(dist.reshape(-1), inside.reshape(-1), jobs, V)
    assert depth.shape == (2, 3) and pen.shape == (2, 3)
    assert np.array_equal(depth, np.asarray([[0.0125, 0.0, 0.03], [0.002, 0.0, 0.0]]) * 100.0)  # centimetres
    assert pen.tolist() == [[True, False, True], [True, True, False]]
    s = PD.summary(depth[0], depth[1], pen[0], pen[1])
    assert s["gt_pd"] == float(np.mean(depth[0])) and s["gt_pd_max"] == 3.0 and s["refined_pd_max"] == 0.2
    assert s["gt_pen_frame_ratio"] == 2 / 3 and s["refined_pen_frame_ratio"] == 2 / 3
    assert set(s) == {"gt_pd", "refined_pd", "gt_pd_max", "refined_pd_max", "gt_pen_frame_ratio", "refined_pen_frame_ratio"}


def test_clip_without_frames_or_meshes_needs_no_gpu():
    hv = np.zeros((30, 5, 3), np.float32)
    traj = np.zeros((1, 30, 9), np.float32)
    traj[..., 3] = traj[..., 7] = 1
    depth, pen = PD.clip_pd(hv, hv, traj, None, [None], 30)
    assert depth.tolist() == [[0.0, 0.0], [0.0, 0.0]] and not pen.any()
    depth, pen = PD.clip_pd(hv, hv, traj, None, [0], 0)
    assert depth.shape == (2, 0) and pen.shape == (2, 0)


def test_penetration_colors():
    import torch

    from oakink2_tamf_amd import render as R

    base, hot = (0.9, 0.7, 0.6), (0.5, 0.1, 0.8)
    depth = np.asarray([0.0, 0.005, 0.01, 0.02, 0.02, 0.004])
    inside = np.asarray([1, 1, 1, 1, 0, 0], bool)
    c = R.penetration_colors(depth, inside, base, hot=hot, far=0.01)
    assert c.dtype == np.float32 and c.shape == (6, 3)
    b, h = np.asarray(base, np.float32), np.asarray(hot, np.float32)
    assert np.array_equal(c[0], b) and np.array_equal(c[2], h) and np.array_equal(c[3], h) and np.array_equal(c[4], b) and np.array_equal(c[5], b)
    assert np.array_equal(c[1], np.float32(0.5) * b + np.float32(0.5) * h)
    t = R.penetration_colors(torch.from_numpy(depth), torch.from_numpy(inside), base, hot=hot, far=0.01)
    assert t.dtype == torch.float32 and np.array_equal(t.numpy(), c)
    with pytest.raises(ValueError, match="far must be positive"):
        R.penetration_colors(depth, inside, base, far=0.0)
