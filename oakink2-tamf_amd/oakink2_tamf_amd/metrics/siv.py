"""Solid Intersection Volume of hand and objects (reference script/compute_score/compute_score_siv.py:128-155,279-299;
dev_fn/util/sdf_util.py:59-99 process_sdf).

An object is voxelised once: a `resolution`^3 lattice over its expanded bounding box, of which the interior points are kept.  Per
sampled frame (every 20th) and hand (ground truth, refined) those points are moved to the frame's pose and counted inside the closed
hand mesh; SIV = count x voxel volume x 1e6 (cm^3), summed over the clip's objects.

The reference takes the lattice's sign from pysdf (`SDF(...)(points) > 0`).  pysdf does not ship here: `object_lattice` uses the
reference's own inside test, check_mesh_contains, instead (geometry.voxelize_lattice).  The two agree away from the surface; lattice
points within rounding of it may differ, and that difference has not been measured.  `load_sdf_pickle` reads voxel sets written by
the reference itself, for whoever has pysdf and wants its exact sets.

The host arithmetic restates the reference's numpy lines in their order and dtypes; the counting is one launch of
geometry.mesh_contains_count for all frames, both hands and all objects of a clip."""
from __future__ import annotations

import pickle
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

STRIDE = 20  # compute_score_siv.py:286


@dataclass
class ObjectLattice:
    """What the SIV score uses of the reference's SDFData, plus the lattice's axes"""
    mesh_center: np.ndarray      # (3,) mean of the 8 corners of the axis-aligned bounding box
    extent: np.ndarray           # (3,) of the centred mesh
    extent_expanded: np.ndarray  # (3,) extent * bbox_expand_ratio
    tick_unit: np.ndarray        # (3,) extent_expanded / resolution  (NOT the linspace spacing, which divides by resolution - 1)
    ticks: Optional[np.ndarray]  # (R, 3) np.linspace(-extent_expanded / 2, extent_expanded / 2, R); None when read from a pickle
    points_in: np.ndarray        # (n, 3) float64: `point[sdf > 0] + mesh_center` of the reference, ascending lattice order
    el_vol: float                # prod(tick_unit)
    resolution: int
    bbox_expand_ratio: float


def _aabb_corners(lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """the 8 corners, x slowest (the vertex order of a box primitive)"""
    b = (lo, hi)
    return np.array([[b[i][0], b[j][1], b[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64)


def lattice_axes(verts, bbox_expand_ratio: float = 1.2, resolution: int = 100) -> Dict:
    """The host half of process_sdf (sdf_util.py:60-74), float64: centre, centred vertices, extents, tick_unit, ticks."""
    v = np.asarray(verts, dtype=np.float64)
    aabb = _aabb_corners(v.min(axis=0), v.max(axis=0))
    center = np.mean(aabb, axis=0)
    centred = v - center
    extent = np.asarray(centred.max(axis=0) - centred.min(axis=0))
    extent_expanded = extent * bbox_expand_ratio
    tick_unit = extent_expanded / resolution
    ticks = np.linspace(-extent_expanded / 2.0, extent_expanded / 2.0, resolution)
    return {"mesh_center": center, "verts_centred": centred, "extent": extent, "extent_expanded": extent_expanded, "tick_unit": tick_unit,
            "ticks": ticks}


def lattice_points(ticks: np.ndarray, mesh_center: np.ndarray, flat_index: np.ndarray) -> np.ndarray:
    """`point[idx] + mesh_center` for flat lattice indices idx = (i * R + j) * R + k, where point = query_point + mesh_center is the
    SDFData field (sdf_util.py:82): the reference adds the centre a second time when it scores (compute_score_siv.py:141-142), and so
    does this."""
    R = ticks.shape[0]
    idx = np.asarray(flat_index, dtype=np.int64)
    q = np.stack([ticks[idx // (R * R), 0], ticks[(idx // R) % R, 1], ticks[idx % R, 2]], axis=1)
    return (q + mesh_center) + mesh_center


def object_lattice(verts, faces, bbox_expand_ratio: float = 1.2, resolution: int = 100, device=None, sign: str = "parity") -> ObjectLattice:
    """process_sdf with the reference's check_mesh_contains as the sign (module docstring).  verts (V,3), faces (F,3) of a closed mesh.
    sign="winding": the voxel set is that of the generalized winding number (winding.lattice_winding, |w| > 0.5), which needs no
    closed mesh and equals the default on a clean closed one."""
    import torch

    from ..geometry import voxelize_lattice
    from ..winding import check_sign, lattice_winding

    check_sign(sign)

    ax = lattice_axes(verts, bbox_expand_ratio, resolution)
    tk = torch.from_numpy(np.ascontiguousarray(ax["ticks"]))
    if device is not None:
        tk = tk.to(device)
    if sign == "parity":
        mask = voxelize_lattice(ax["verts_centred"], np.asarray(faces), tk)
    else:
        mask = lattice_winding(ax["verts_centred"], np.asarray(faces), tk, device=device)[1]
    idx = torch.nonzero(mask.reshape(-1)).reshape(-1).cpu().numpy()  # ascending
    return ObjectLattice(mesh_center=ax["mesh_center"], extent=ax["extent"], extent_expanded=ax["extent_expanded"], tick_unit=ax["tick_unit"],
                         ticks=ax["ticks"], points_in=lattice_points(ax["ticks"], ax["mesh_center"], idx),
                         el_vol=float(np.prod(ax["tick_unit"])), resolution=int(resolution), bbox_expand_ratio=float(bbox_expand_ratio))


def load_sdf_pickle(path: str) -> ObjectLattice:
    """A voxel set written by the reference: the pickled dict of the SDFData fields that sdf_util.load_sdf_data reads."""
    with open(path, "rb") as f:
        d = pickle.load(f)
    point, sdf = np.asarray(d["point"], dtype=np.float64), np.asarray(d["sdf"])
    center, tick_unit = np.asarray(d["mesh_center"], dtype=np.float64), np.asarray(d["tick_unit"], dtype=np.float64)
    ee = d.get("extent_expanded")
    return ObjectLattice(mesh_center=center, extent=np.asarray(d.get("extent", np.full(3, np.nan)), dtype=np.float64),
                         extent_expanded=np.asarray(ee if ee is not None else np.full(3, np.nan), dtype=np.float64), tick_unit=tick_unit,
                         ticks=None, points_in=point[sdf > 0] + center, el_vol=float(np.prod(tick_unit)),
                         resolution=int(d.get("resolution", round(len(point) ** (1.0 / 3.0)))),
                         bbox_expand_ratio=float(d.get("bbox_expand_ratio", float("nan"))))


def tslrot6d_to_transf(tslrot6d: np.ndarray) -> np.ndarray:
    """(..., 9) -> (..., 4, 4) in the input's dtype (float32 in the score): tslrot6d_to_transf_np (transform_np.py:169-175) with
    rot6d_to_rotmat_np (rotation_np.py:471-499: v / max(|v|, eps of the dtype); rows b1, b2, b1 x b2)."""
    x = np.asarray(tslrot6d)
    eps = np.finfo(x.dtype).eps
    a1, a2 = x[..., 3:6], x[..., 6:9]
    b1 = a1 / np.maximum(np.linalg.norm(a1, ord=2, axis=-1, keepdims=True), eps)
    b2 = a2 - np.sum(b1 * a2, axis=-1, keepdims=True) * b1
    b2 = b2 / np.maximum(np.linalg.norm(b2, ord=2, axis=-1, keepdims=True), eps)
    b3 = np.cross(b1, b2, axis=-1)
    res = np.zeros(x.shape[:-1] + (4, 4), dtype=x.dtype)
    res[..., 3, 3] = 1.0
    res[..., :3, 3] = x[..., 0:3]
    res[..., :3, :3] = np.stack((b1, b2, b3), axis=-2)
    return res


def clip_jobs(avai_len: int, n_points: Sequence[Optional[int]], stride: int = STRIDE) -> Dict[str, np.ndarray]:
    """The job list of one clip.  n_points[o]: interior points of object o, None for an object without a lattice (skipped, as
    `if obj_id not in obj_sdf_map: continue`).  Order: frames range(0, avai_len, stride); per frame the ground-truth hand, then the
    refined one; per hand the objects in the clip's order.  Mesh 2 f + h is hand h of sampled frame f; the objects' points lie end to
    end in the clip's order.  Every entry of n_points is scored: the ids behind them are taken to be distinct, as the dataset's obj_list
    is (the reference keys a frame's transforms by id, so it would score a repeated id once; the launcher refuses such a clip).
    -> frames (n,), and per job: frame_slot, hand, obj, mesh_id, pt_off, pt_len"""
    frames = np.arange(0, int(avai_len), int(stride), dtype=np.int64)
    kept = [o for o, n in enumerate(n_points) if n is not None]
    off = {}
    acc = 0
    for o in kept:
        off[o] = acc
        acc += int(n_points[o])
    slot, hand, obj = [], [], []
    for f in range(len(frames)):
        for h in (0, 1):
            for o in kept:
                slot.append(f)
                hand.append(h)
                obj.append(o)
    slot, hand, obj = (np.asarray(a, dtype=np.int64) for a in (slot, hand, obj))
    return {"frames": frames, "frame_slot": slot, "hand": hand, "obj": obj, "mesh_id": (2 * slot + hand).astype(np.int32),
            "pt_off": np.asarray([off[o] for o in obj], dtype=np.int64), "pt_len": np.asarray([int(n_points[o]) for o in obj], dtype=np.int64)}


def clip_siv(hand_verts_gt, hand_verts_refined, faces_closed, obj_traj, lattices: Sequence[Optional[ObjectLattice]], avai_len: int,
             stride: int = STRIDE, device=None) -> Tuple[List[float], List[float]]:
    """SIV in cm^3 of every sampled frame of one clip, (ground truth, refined).  hand_verts_* (T, V, 3) float32, faces_closed (F, 3),
    obj_traj (nobj, T, 9) = [tsl | rot6d] (float32 in the dataset), lattices[o] the object's ObjectLattice or None."""
    import torch

    from ..geometry import mesh_contains_count

    avai_len = int(avai_len)
    jobs = clip_jobs(avai_len, [None if l is None else len(l.points_in) for l in lattices], stride)
    frames = jobs["frames"]
    n = len(frames)
    if n == 0 or len(jobs["mesh_id"]) == 0:
        return [0.0] * n, [0.0] * n
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    gt = np.asarray(hand_verts_gt, dtype=np.float32)[:avai_len][frames]
    rf = np.asarray(hand_verts_refined, dtype=np.float32)[:avai_len][frames]
    hands = torch.from_numpy(np.ascontiguousarray(np.stack([gt, rf], axis=1).reshape(2 * n, gt.shape[1], 3))).to(dev)
    transf = tslrot6d_to_transf(np.asarray(obj_traj)[:, :avai_len])  # (nobj, len, 4, 4), the reference's matrices
    tr = transf[jobs["obj"], frames[jobs["frame_slot"]], :3, :].astype(np.float64)  # upcast: exact
    points = torch.from_numpy(np.ascontiguousarray(np.concatenate([l.points_in for l in lattices if l is not None], axis=0))).to(dev)
    count = mesh_contains_count(hands, faces_closed, points, jobs["pt_off"], jobs["pt_len"], jobs["mesh_id"], tr).cpu().numpy()
    el_vol = np.asarray([0.0 if l is None else l.el_vol for l in lattices])
    out = ([0.0] * n, [0.0] * n)
    for c, f, h, o in zip(count, jobs["frame_slot"], jobs["hand"], jobs["obj"]):  # objects ascending within (frame, hand): the reference's order
        out[h][f] += c * el_vol[o] * (10 ** 6)
    return out


__all__ = ["STRIDE", "ObjectLattice", "lattice_axes", "lattice_points", "object_lattice", "load_sdf_pickle", "tslrot6d_to_transf",
           "clip_jobs", "clip_siv"]
