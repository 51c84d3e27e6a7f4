"""Penetration depth of hand into objects: how DEEP the hand goes, beside SIV's how much volume (metrics/siv.py).

Per sampled frame (every 20th of the first `len` frames, the frames SIV scores) and hand (ground truth, refined) every hand vertex is
taken into each object's frame by the inverse of the frame's pose, and measured against the object's mesh with the exact point-to-mesh
distance of libtamf_meshdist.so (meshdist.py, include/tamf_meshdist.h).  A frame's depth is the largest distance over the objects and
over the vertices that lie inside (the reference's check_mesh_contains, as in SIV), 0 when no vertex is inside; in centimetres, as SIV
is in cm^3.  All jobs of a clip go through one tamf_meshdist_points call.

The pose is metrics/siv.tslrot6d_to_transf's matrix in the dataset's dtype (float32), as SIV uses it; its inverse R^T, -(R^T t) is taken
on the host in that dtype and then widened to float64, which is exact.  The reference has no such score: the definition is this
package's, the standard one of the hand-object literature."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .siv import STRIDE, tslrot6d_to_transf

CM = 100.0  # metres -> centimetres


def inverse_transf(transf: np.ndarray) -> np.ndarray:
    """(..., 4, 4) rigid -> (..., 3, 4) rows of [R^T | -(R^T t)] in the input's dtype"""
    t = np.asarray(transf)
    rt = np.swapaxes(t[..., :3, :3], -1, -2)
    ti = -np.matmul(rt, t[..., :3, 3:4])
    return np.concatenate([rt, ti], axis=-1)


def clip_jobs(avai_len: int, mesh_ids: Sequence[Optional[int]], n_verts: int, stride: int = STRIDE) -> Dict[str, np.ndarray]:
    """The job list of one clip.  mesh_ids[o]: the object's mesh in the MeshSet, None for an object without a mesh (left out).  Order,
    as metrics/siv.clip_jobs: frames range(0, avai_len, stride); per frame the ground-truth hand, then the refined one; per hand the
    objects in the clip's order.  The hand vertices lie (frame, hand)-major: hand h of sampled frame f at rows (2 f + h) n_verts.
    -> frames (n,), and per job: frame_slot, hand, obj, mesh_id, pt_off, pt_len"""
    frames = np.arange(0, int(avai_len), int(stride), dtype=np.int64)
    kept = [o for o, m in enumerate(mesh_ids) if m is not None]
    slot, hand, obj = [], [], []
    for f in range(len(frames)):
        for h in (0, 1):
            for o in kept:
                slot.append(f)
                hand.append(h)
                obj.append(o)
    slot, hand, obj = (np.asarray(a, dtype=np.int64) for a in (slot, hand, obj))
    return {"frames": frames, "frame_slot": slot, "hand": hand, "obj": obj,
            "mesh_id": np.asarray([mesh_ids[o] for o in obj], dtype=np.int32), "pt_off": (2 * slot + hand) * int(n_verts),
            "pt_len": np.full(len(obj), int(n_verts), dtype=np.int64)}


def reduce_frames(dist, inside, jobs: Dict[str, np.ndarray], n_verts: int) -> Tuple[np.ndarray, np.ndarray]:
    """dist (J * n_verts,) metres and inside (J * n_verts,) bool in job order -> depth (2, n_frames) in CENTIMETRES (row 0 the ground
    truth, row 1 the refined hand): the largest distance among a frame's inside vertices over its objects, 0 when there is none; and
    penetrating (2, n_frames) bool: whether any vertex was inside."""
    n = len(jobs["frames"])
    J = len(jobs["mesh_id"])
    d = np.asarray(dist, dtype=np.float64).reshape(J, int(n_verts))
    m = np.asarray(inside, dtype=bool).reshape(J, int(n_verts))
    per_job = np.where(m, d, 0.0).max(axis=1) if J else np.zeros(0)
    any_job = m.any(axis=1) if J else np.zeros(0, bool)
    depth, pen = np.zeros((2, n)), np.zeros((2, n), dtype=bool)
    for j in range(J):
        h, f = int(jobs["hand"][j]), int(jobs["frame_slot"][j])
        depth[h, f] = max(depth[h, f], per_job[j])
        pen[h, f] |= bool(any_job[j])
    return depth * CM, pen


def clip_pd(hand_verts_gt, hand_verts_refined, obj_traj, mesh_set, mesh_ids: Sequence[Optional[int]], avai_len: int, stride: int = STRIDE,
            cull: bool = True, sign: str = "parity", winding_set=None) -> Tuple[np.ndarray, np.ndarray]:
    """Penetration depth of every sampled frame of one clip -> depth (2, n_frames) in cm, penetrating (2, n_frames) bool; row 0 the
    ground-truth hand, row 1 the refined one.  hand_verts_* (T, V, 3) float32, obj_traj (nobj, T, 9) = [tsl | rot6d] (float32 in the
    dataset), mesh_set a meshdist.MeshSet, mesh_ids[o] the clip's object o in it or None (no mesh: left out).
    sign="winding": `inside` comes from winding_set (a winding.WindingSet of the same meshes in the same order) on the same jobs and
    transforms - the generalized winding number, for object meshes that are not closed; the distance is mesh_set's as before."""
    from ..winding import check_sign

    if check_sign(sign) == "winding" and winding_set is None:
        raise ValueError("clip_pd: sign='winding' needs winding_set, a winding.WindingSet of mesh_set's meshes")
    avai_len = int(avai_len)
    gt = np.asarray(hand_verts_gt, dtype=np.float32)[:avai_len]
    rf = np.asarray(hand_verts_refined, dtype=np.float32)[:avai_len]
    V = int(gt.shape[1])
    jobs = clip_jobs(avai_len, mesh_ids, V, stride)
    frames = jobs["frames"]
    n = len(frames)
    if n == 0 or len(jobs["mesh_id"]) == 0:
        return np.zeros((2, n)), np.zeros((2, n), dtype=bool)
    hands = np.ascontiguousarray(np.stack([gt[frames], rf[frames]], axis=1).reshape(2 * n * V, 3))
    inv = inverse_transf(tslrot6d_to_transf(np.asarray(obj_traj)[:, :avai_len]))  # (nobj, len, 3, 4), the dataset's dtype
    tr = inv[jobs["obj"], frames[jobs["frame_slot"]]].astype(np.float64)  # upcast: exact
    dist, _, inside = mesh_set.distance(hands, jobs["mesh_id"], tr, jobs["pt_off"], jobs["pt_len"], inside=sign == "parity", cull=cull)
    if sign == "winding":
        _, inside = winding_set.points(hands, jobs["mesh_id"], tr, jobs["pt_off"], jobs["pt_len"], inside=True)
    return reduce_frames(dist.cpu().numpy(), inside.cpu().numpy(), jobs, V)


def summary(gt_depth: Sequence[float], refined_depth: Sequence[float], gt_pen: Sequence[bool], refined_pen: Sequence[bool]) -> Dict[str, float]:
    """the figures of the score over all frames: means and maxima in cm, and the share of frames with any vertex inside"""
    g, r = np.asarray(gt_depth, dtype=np.float64), np.asarray(refined_depth, dtype=np.float64)
    return {"gt_pd": float(g.mean()), "refined_pd": float(r.mean()), "gt_pd_max": float(g.max()), "refined_pd_max": float(r.max()),
            "gt_pen_frame_ratio": float(np.mean(np.asarray(gt_pen, dtype=bool))), "refined_pen_frame_ratio": float(np.mean(np.asarray(refined_pen, dtype=bool)))}


__all__ = ["STRIDE", "CM", "inverse_transf", "clip_jobs", "reduce_frames", "clip_pd", "summary"]
