"""Torch restatement (float64 or float32, any device, with autograd) of what contact.py and model/interaction_loss.py compute, written
from the semantics: the signed point-to-point distance between two clouds in both directions (each point's nearest neighbour in the
other cloud by squared euclidean distance, an `argmin`, lowest index on a tie; the object-to-hand distance signed by the side of the
nearest hand vertex's normal the point lies on), per clip, object and frame; and the two loss terms built on it.  Test infrastructure:
the reference of tests/test_contact_*.py and the baseline of tools/contact_bench.py."""
from __future__ import annotations

import numpy as np
import torch

W_FAR = float(np.float32(0.1))  # the weights tensor of the loss this restates is float32 whatever the inputs' dtype


def unit(v):
    return v / torch.linalg.vector_norm(v, dim=-1, keepdim=True).clamp_min(1e-12)


def rot6d_rows(d6):
    """(..., 6) -> (..., 3, 3): Gram-Schmidt of the two 3-vectors into the first two rows, their cross product the third"""
    a, b = d6[..., :3], d6[..., 3:]
    r0 = unit(a)
    r1 = unit(b - r0 * (r0 * b).sum(-1, keepdim=True))
    return torch.stack([r0, r1, torch.linalg.cross(r0, r1)], dim=-2)


def move_points(obj_traj, obj_points):
    """obj_traj (..., T, 9) = tsl | rot6d, obj_points (..., P, 3) -> (..., T, P, 3): y = R p + t per frame"""
    R = rot6d_rows(obj_traj[..., 3:])
    return torch.einsum("...tij,...pj->...tpi", R, obj_points) + obj_traj[..., None, :3]


def vertex_normals(verts, faces):
    """verts (..., V, 3), faces (F, 3) -> (..., V, 3): every face adds its area-weighted normal to its three corners; the sums are
    normalised as x / max(|x|, 1e-6) (the published vertex-normal rule of pytorch3d's meshes)"""
    faces = torch.as_tensor(faces, device=verts.device).long()
    v0, v1, v2 = (verts[..., faces[:, k], :] for k in range(3))
    n = torch.zeros_like(verts)
    n = n.index_add(-2, faces[:, 1], torch.linalg.cross(v2 - v1, v0 - v1))
    n = n.index_add(-2, faces[:, 2], torch.linalg.cross(v0 - v2, v1 - v2))
    n = n.index_add(-2, faces[:, 0], torch.linalg.cross(v1 - v0, v2 - v0))
    return n / torch.linalg.vector_norm(n, dim=-1, keepdim=True).clamp_min(1e-6)


def sq_dists(x, y):
    """x (..., A, 3), y (..., C, 3) -> (..., A, C) squared distances, by broadcast (no cdist: no cancellation)"""
    return ((x[..., :, None, :] - y[..., None, :, :]) ** 2).sum(-1)


def point2point_signed(x, y, x_normals=None):
    """x (N, A, 3), y (N, C, 3), x_normals (N, A, 3) or None -> (y2x_signed (N, C), x2y (N, A), yidx (N, C), xidx (N, A))"""
    d2 = sq_dists(x, y)
    xidx, yidx = d2.argmin(dim=-1), d2.argmin(dim=-2)
    x2y = x - torch.gather(y, 1, xidx[..., None].expand(-1, -1, 3))
    y2x = y - torch.gather(x, 1, yidx[..., None].expand(-1, -1, 3))
    y2x_signed = torch.linalg.vector_norm(y2x, dim=-1)
    if x_normals is not None:
        n = torch.gather(x_normals, 1, yidx[..., None].expand(-1, -1, 3))
        y2x_signed = y2x_signed * (n * y2x).sum(-1).sign()
    return y2x_signed, torch.linalg.vector_norm(x2y, dim=-1), yidx, xidx


def contact_all(hand_verts, hand_normals, obj_traj, obj_points, obj_num=None, want_o2h=True):
    """-> (o2h_signed (B,nobj,T,P), h2o (B,nobj,T,V), o2h_idx (B,nobj,T,P) int32, h2o_idx (B,nobj,T,V) int32) per object; rows of padded
    objects are 0, with index -1"""
    B, T, V, _ = hand_verts.shape
    nobj, P = obj_points.shape[1], obj_points.shape[2]
    moved = move_points(obj_traj, obj_points)  # (B, nobj, T, P, 3)
    o2h, h2o, o2h_idx, h2o_idx = [], [], [], []
    for b in range(B):
        n = nobj if obj_num is None else int(obj_num[b])
        for o in range(nobj):
            if o >= n:
                z = hand_verts.new_zeros
                o2h.append(z(T, P)), h2o.append(z(T, V)), o2h_idx.append(z(T, P, dtype=torch.int32) - 1), h2o_idx.append(z(T, V, dtype=torch.int32) - 1)
                continue
            a, c, ai, ci = point2point_signed(hand_verts[b], moved[b, o], None if hand_normals is None else hand_normals[b])
            o2h.append(a), h2o.append(c), o2h_idx.append(ai.to(torch.int32)), h2o_idx.append(ci.to(torch.int32))
    sh = lambda lst, n: torch.stack(lst).reshape(B, nobj, T, n)  # noqa: E731
    if not want_o2h:
        return None, sh(h2o, V), None, sh(h2o_idx, V)
    return sh(o2h, P), sh(h2o, V), sh(o2h_idx, P), sh(h2o_idx, V)


def signed_contact_distance(hand_verts, hand_normals, obj_traj, obj_points, obj_num=None, want_o2h=True):
    """the signature and the results of contact.signed_contact_distance"""
    return contact_all(hand_verts, hand_normals, obj_traj, obj_points, obj_num, want_o2h)[:3]


def merged_h2o_dist(hand_verts, obj_traj, obj_points, obj_num=None):
    """(B, T, V): distance to the nearest point of all real objects of the clip, merged into one cloud"""
    B, T = hand_verts.shape[:2]
    moved = move_points(obj_traj, obj_points)
    out = []
    for b in range(B):
        n = obj_points.shape[1] if obj_num is None else int(obj_num[b])
        cloud = moved[b, :n].permute(1, 0, 2, 3).reshape(T, -1, 3)
        out.append(point2point_signed(hand_verts[b], cloud)[1])
    return torch.stack(out)


def conditions(hand_verts, hand_normals, obj_traj, obj_points, obj_num=None):
    """How far the inputs are from a decision that rounding could flip, over the real objects: -> (the smallest relative gap between
    the nearest and the second-nearest squared distance of any query, both directions; the smallest |cos(n, y - x_near)| of the
    sign, 1.0 without normals).  A direction with one candidate only has no second-nearest and is left out."""
    B = hand_verts.shape[0]
    nobj = obj_points.shape[1]
    moved = move_points(obj_traj, obj_points)
    gap, cos = float("inf"), 1.0
    for b in range(B):
        for o in range(nobj if obj_num is None else int(obj_num[b])):
            d2 = sq_dists(hand_verts[b], moved[b, o])  # (T, V, P)
            for dim in (-1, -2):
                if d2.shape[dim] > 1:
                    two = torch.topk(d2, 2, dim=dim, largest=False).values
                    lo, hi = two.select(dim, 0), two.select(dim, 1)
                    gap = min(gap, float(((hi - lo) / hi.clamp_min(1e-300)).min()))
            if hand_normals is not None:
                yidx = d2.argmin(dim=-2)
                y2x = moved[b, o] - torch.gather(hand_verts[b], 1, yidx[..., None].expand(-1, -1, 3))
                n = torch.gather(hand_normals[b], 1, yidx[..., None].expand(-1, -1, 3))
                c = (n * y2x).sum(-1).abs() / (torch.linalg.vector_norm(n, dim=-1) * torch.linalg.vector_norm(y2x, dim=-1)).clamp_min(1e-300)
                cos = min(cos, float(c.min()))
    return gap, cos


def point_weights(o2h_signed, o2h_signed_gt):
    """the per-point weights of `dist_o`: 1, then 0.1 outside the window -0.005 < ground truth < 0.01, then 1.5 where the prediction
    penetrates - in that order"""
    w = torch.ones_like(o2h_signed_gt)
    w[~((o2h_signed_gt < 0.01) & (o2h_signed_gt > -0.005))] = W_FAR
    w[o2h_signed.detach() < 0.0] = 1.5
    return w


def dist_terms(verts_pred, normals_pred, verts_gt, normals_gt, obj_traj, obj_points, obj_num, mask, v_weights2):
    """the segment loss's `dist_h`, `dist_o`, each summed over the clips: per clip b and real object o, with c_b = T / sum(mask_b),
        dist_h += c_b * mean over (t, v) of | |h2o| - |h2o_gt| | * v_weights2[v] * mask[t]  / num_obj_b
        dist_o += c_b * mean over (t, j) of | o2h_signed - o2h_signed_gt | * w[t, j] * mask[t]  / num_obj_b"""
    B, T = mask.shape
    o2h, h2o, _ = signed_contact_distance(verts_pred, normals_pred, obj_traj, obj_points, obj_num)
    with torch.no_grad():
        o2h_g, h2o_g, _ = signed_contact_distance(verts_gt, normals_gt, obj_traj, obj_points, obj_num)
    dist_h = dist_o = 0.0
    for b in range(B):
        n = obj_points.shape[1] if obj_num is None else int(obj_num[b])
        c = float(T) / float(mask[b].sum())
        for o in range(n):
            w = point_weights(o2h[b, o], o2h_g[b, o])
            dist_h = dist_h + c * ((h2o[b, o].abs() - h2o_g[b, o].abs()).abs() * v_weights2 * mask[b][:, None]).mean() / n
            dist_o = dist_o + c * ((o2h[b, o] - o2h_g[b, o]).abs() * w * mask[b][:, None]).mean() / n
    return dist_h, dist_o


def refine_dist_h(refine_h2o, target_h2o, mask, v_weights2):
    """the refine loss's `dist_h`: the mean over the clips of c_b * mean over (t, v) of | |refine| - |target| | * mask[t] * v_weights2[v]"""
    e = (refine_h2o.abs() - target_h2o.abs()).abs() * mask[..., None] * v_weights2
    return ((float(mask.shape[1]) / mask.sum(dim=1)) * e.mean(dim=(-2, -1))).mean()
