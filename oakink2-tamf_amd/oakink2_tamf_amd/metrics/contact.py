"""Contact Ratio (reference script/compute_score/compute_score_cr.py:268-285): the per-frame hand-object contact distance of every
valid frame of every clip, batched into geometry.contact_min_dist (HIP, tamf_contact_min_dist), and the share of frames below 5 mm."""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np

THRESHOLD = 0.005  # :282-283


def contact_distances(items: Sequence[Dict], verts: Sequence, batch_size: int = 64, device="cuda:0") -> np.ndarray:
    """items: dataset items (`len`, `obj_traj` (nobj, T, 9), `obj_pointcloud` (nobj, P, 3)); verts[i] (T, V, 3) the hand vertices of
    item i.  Clips of equal (T, V, P) are batched - the object axis zero-padded to the batch maximum, the kernel told each clip's own
    count - and the first `len` frames of each clip are kept (the reference slices before it measures, :269-271; a frame's distance
    does not depend on the other frames).  -> float32 (sum of len,) in item order: what the reference `extend`s into
    `gt_contact_dist` / `refined_contact_dist`."""
    import torch

    from ..geometry import contact_min_dist

    if len(items) != len(verts):
        raise ValueError(f"contact_distances: {len(items)} items, {len(verts)} vertex arrays")
    out: List = [None] * len(items)
    groups: Dict = {}
    for i, (it, v) in enumerate(zip(items, verts)):
        traj, pc = np.asarray(it["obj_traj"]), np.asarray(it["obj_pointcloud"])
        v = np.asarray(v)
        if traj.shape[0] != pc.shape[0] or traj.shape[1] != v.shape[0]:
            raise ValueError(f"contact_distances: clip {i}: obj_traj {traj.shape}, obj_pointcloud {pc.shape}, verts {v.shape}")
        groups.setdefault((int(v.shape[0]), int(v.shape[1]), int(pc.shape[1])), []).append(i)
    for (T, V, P), idx in groups.items():
        for s in range(0, len(idx), batch_size):
            part = idx[s: s + batch_size]
            nobj = max(int(np.asarray(items[i]["obj_traj"]).shape[0]) for i in part)
            hv = np.stack([np.asarray(verts[i], dtype=np.float32) for i in part], axis=0)
            traj = np.zeros((len(part), nobj, T, 9), np.float32)
            pts = np.zeros((len(part), nobj, P, 3), np.float32)
            obj_num = []
            for b, i in enumerate(part):
                t_i, p_i = np.asarray(items[i]["obj_traj"], dtype=np.float32), np.asarray(items[i]["obj_pointcloud"], dtype=np.float32)
                traj[b, : t_i.shape[0]] = t_i
                pts[b, : p_i.shape[0]] = p_i
                obj_num.append(int(t_i.shape[0]))
            d = contact_min_dist(torch.from_numpy(hv).to(device), torch.from_numpy(traj).to(device), torch.from_numpy(pts).to(device),
                                 obj_num=obj_num).cpu().numpy()
            for b, i in enumerate(part):
                out[i] = d[b, : int(items[i]["len"])]
    return np.concatenate(out, axis=0) if out else np.zeros((0,), np.float32)


def contact_ratio_of(dist: np.ndarray, threshold: float = THRESHOLD) -> float:
    """np.mean(dist < 0.005) (:282-285)"""
    return float(np.mean(np.asarray(dist) < threshold))
