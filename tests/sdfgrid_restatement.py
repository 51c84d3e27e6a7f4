"""THE DEFINITION of include/tamf_sdfgrid.h stated again in numpy float64, one operation per line: depth, cell and g_hand.  numpy's
float64 `+ - * /` and sqrt are IEEE and never fused, so the kernels (compiled with -ffp-contract=off) must give the same bits.

A grid is a dict {"values": (R^3,) float32, "res": R, "origin": (3,) float64, "step": (3,) float64}: what sdfgrid.pack_grid returns.

`depth_torch` is the same quantity in torch ops of any float dtype, for the tests that need autograd through it (its float64 run is
their reference, its float32 run measures what float32 costs); it makes no claim about bits."""
from __future__ import annotations

import numpy as np

EPS = float(np.finfo(np.float32).eps)


def dot3(ux, uy, uz, vx, vy, vz):
    a = ux * vx
    b = uy * vy
    c = uz * vz
    return (a + b) + c


def pose(tr):
    """(..., 9) float32 rows tsl | rot6d -> (R (..., 3, 3) with the rows b1, b2, b3, t (..., 3)), float64"""
    tr = np.asarray(tr, dtype=np.float32).astype(np.float64)
    t = tr[..., 0:3]
    a0, a1, a2, a3, a4, a5 = (tr[..., 3 + k] for k in range(6))
    with np.errstate(all="ignore"):
        n1 = np.sqrt(dot3(a0, a1, a2, a0, a1, a2))
        n1 = np.where(n1 > EPS, n1, EPS)
        b1x = a0 / n1
        b1y = a1 / n1
        b1z = a2 / n1
        dp = dot3(b1x, b1y, b1z, a3, a4, a5)
        b2x = a3 - dp * b1x
        b2y = a4 - dp * b1y
        b2z = a5 - dp * b1z
        n2 = np.sqrt(dot3(b2x, b2y, b2z, b2x, b2y, b2z))
        n2 = np.where(n2 > EPS, n2, EPS)
        b2x = b2x / n2
        b2y = b2y / n2
        b2z = b2z / n2
        b3x = b1y * b2z - b1z * b2y
        b3y = b1z * b2x - b1x * b2z
        b3z = b1x * b2y - b1y * b2x
    R = np.stack([np.stack([b1x, b1y, b1z], -1), np.stack([b2x, b2y, b2z], -1), np.stack([b3x, b3y, b3z], -1)], -2)
    return R, t


def object_frame(R, t, x):
    """p_k = (R_0k d_0 + R_1k d_1) + R_2k d_2, d = x - t; R (..., 3, 3), t (..., 3) broadcast against x (..., 3) float32"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        d0 = x[..., 0] - t[..., 0]
        d1 = x[..., 1] - t[..., 1]
        d2 = x[..., 2] - t[..., 2]
        p = [(R[..., 0, k] * d0 + R[..., 1, k] * d1) + R[..., 2, k] * d2 for k in range(3)]
    return np.stack(p, -1)


def sample(grid, R, t, x):
    """One lattice under the poses (R, t) at the vertices x -> (s (...) float64 where positive else 0, cell (...) int32 or -1,
    w (..., 3) float64 world gradient, 0 where s is not positive)"""
    res = int(grid["res"])
    vals = np.asarray(grid["values"], dtype=np.float32).astype(np.float64)
    og = np.asarray(grid["origin"], dtype=np.float64)
    st = np.asarray(grid["step"], dtype=np.float64)
    p = object_frame(R, t, x)
    with np.errstate(all="ignore"):
        u = [(p[..., k] - og[k]) / st[k] for k in range(3)]
        hi = float(res - 1)
        ok = np.ones(p.shape[:-1], dtype=bool)
        for k in range(3):
            ok &= (u[k] >= 0.0) & (u[k] <= hi)
        u = [np.where(ok, u[k], 0.0) for k in range(3)]
        i = [np.minimum(np.floor(u[k]).astype(np.int64), res - 2) for k in range(3)]
        fx = u[0] - i[0].astype(np.float64)
        fy = u[1] - i[1].astype(np.float64)
        fz = u[2] - i[2].astype(np.float64)
        c = (i[0] * res + i[1]) * res + i[2]
        rr = res * res
        s000, s001, s010, s011 = vals[c], vals[c + 1], vals[c + res], vals[c + res + 1]
        s100, s101, s110, s111 = vals[c + rr], vals[c + rr + 1], vals[c + rr + res], vals[c + rr + res + 1]
        d00 = s001 - s000
        d01 = s011 - s010
        d10 = s101 - s100
        d11 = s111 - s110
        c00 = s000 + d00 * fz
        c01 = s010 + d01 * fz
        c10 = s100 + d10 * fz
        c11 = s110 + d11 * fz
        e0 = c01 - c00
        e1 = c11 - c10
        c0 = c00 + e0 * fy
        c1 = c10 + e1 * fy
        gx = c1 - c0
        s = c0 + gx * fx
        pos = ok & (s > 0.0)
        gy = e0 + (e1 - e0) * fx
        m0 = d00 + (d01 - d00) * fy
        m1 = d10 + (d11 - d10) * fy
        gz = m0 + (m1 - m0) * fx
        q0 = gx / st[0]
        q1 = gy / st[1]
        q2 = gz / st[2]
        w = [(R[..., r, 0] * q0 + R[..., r, 1] * q1) + R[..., r, 2] * q2 for r in range(3)]
    w = np.stack([np.broadcast_to(wr, pos.shape) for wr in w], -1)
    return np.where(pos, s, 0.0), np.where(pos, c, -1).astype(np.int32), np.where(pos[..., None], w, 0.0), pos


def _grid_of(grids, grid_id, obj_num, b, o):
    if obj_num is not None and o >= int(obj_num[b]):
        return None
    g = int(grid_id[b][o])
    if g < 0 or g >= len(grids) or not 2 <= int(grids[g]["res"]) <= 512:
        return None
    return grids[g]


def forward(grids, hand_verts, obj_traj, grid_id, obj_num=None):
    """-> depth (B, nobj, T, V) float32, cell (B, nobj, T, V) int32"""
    hand = np.asarray(hand_verts, dtype=np.float32)
    traj = np.asarray(obj_traj, dtype=np.float32)
    B, T, V, _ = hand.shape
    nobj = traj.shape[1]
    depth = np.zeros((B, nobj, T, V), np.float32)
    cell = np.full((B, nobj, T, V), -1, np.int32)
    for b in range(B):
        for o in range(nobj):
            grid = _grid_of(grids, grid_id, obj_num, b, o)
            if grid is None:
                continue
            R, t = pose(traj[b, o])  # (T, 3, 3), (T, 3)
            s, c, _, _ = sample(grid, R[:, None], t[:, None], hand[b])
            depth[b, o] = s.astype(np.float32)
            cell[b, o] = c
    return depth, cell


def backward(grids, hand_verts, obj_traj, grid_id, obj_num, g_depth):
    """-> g_hand (B, T, V, 3) float32: the sum over the real objects with a lattice and s > 0, ascending, of g_depth * w"""
    hand = np.asarray(hand_verts, dtype=np.float32)
    traj = np.asarray(obj_traj, dtype=np.float32)
    gd = np.asarray(g_depth, dtype=np.float32).astype(np.float64)
    B, T, V, _ = hand.shape
    nobj = traj.shape[1]
    acc = np.zeros((B, T, V, 3), np.float64)
    for b in range(B):
        for o in range(nobj):
            grid = _grid_of(grids, grid_id, obj_num, b, o)
            if grid is None:
                continue
            R, t = pose(traj[b, o])
            _, _, w, pos = sample(grid, R[:, None], t[:, None], hand[b])
            with np.errstate(all="ignore"):
                term = gd[b, o][..., None] * w
            acc[b] = np.where(pos[..., None], acc[b] + term, acc[b])
    return acc.astype(np.float32)


def penetration_depth(grids):
    """A `pen_fn` for HandInteractionLoss on CPU tensors: the restatement's depth, forward only (no gradient)."""
    import torch

    def fn(hand_verts, obj_traj, grid_id, obj_num=None):
        d, _ = forward(grids, hand_verts.detach().cpu().numpy(), obj_traj.detach().cpu().numpy(), np.asarray(grid_id), obj_num)
        return torch.from_numpy(d).to(hand_verts.device)

    return fn


def depth_torch(grid, hand_verts, traj_rows, dtype):
    """The depth of THE DEFINITION in torch ops of `dtype`, through which autograd passes: hand_verts (..., T, V, 3), traj_rows
    (..., T, 9), one lattice -> (..., T, V)"""
    import torch

    res = int(grid["res"])
    dev = hand_verts.device
    vals = torch.as_tensor(np.asarray(grid["values"], np.float32)).to(device=dev, dtype=dtype)
    og = torch.as_tensor(np.asarray(grid["origin"], np.float64)).to(device=dev, dtype=dtype)
    st = torch.as_tensor(np.asarray(grid["step"], np.float64)).to(device=dev, dtype=dtype)
    x, tr = hand_verts.to(dtype), traj_rows.to(dtype)
    a1, a2 = tr[..., 3:6], tr[..., 6:9]
    b1 = a1 / a1.norm(dim=-1, keepdim=True).clamp_min(EPS)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = b2 / b2.norm(dim=-1, keepdim=True).clamp_min(EPS)
    R = torch.stack([b1, b2, torch.linalg.cross(b1, b2)], dim=-2)  # (..., T, 3, 3), rows
    d = x - tr[..., None, 0:3]
    p = torch.einsum("...trk,...tvr->...tvk", R, d)
    u = (p - og) / st
    ok = ((u >= 0) & (u <= res - 1)).all(dim=-1)
    u = torch.where(ok[..., None], u, torch.zeros_like(u))
    i = u.detach().floor().clamp(max=res - 2).long()
    f = u - i.to(dtype)
    c = (i[..., 0] * res + i[..., 1]) * res + i[..., 2]
    rr = res * res
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]

    def lerp(a, b, w):
        return a + (b - a) * w

    c00, c01 = lerp(vals[c], vals[c + 1], fz), lerp(vals[c + res], vals[c + res + 1], fz)
    c10, c11 = lerp(vals[c + rr], vals[c + rr + 1], fz), lerp(vals[c + rr + res], vals[c + rr + res + 1], fz)
    s = lerp(lerp(c00, c01, fy), lerp(c10, c11, fy), fx)
    return torch.where(ok & (s > 0), s, torch.zeros_like(s))
