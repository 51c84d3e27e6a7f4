"""Case tables and float64 references for the geometry kernels of csrc/tamf_geom.h over their accepted shape ranges (no GPU here;
imported by test_geometry_edges_cpu.py and test_geometry_edges_gpu.py).

References are oracle/geometry_oracle.py called with double tensors; pose decode has ground truth by construction.  `e32` of a
case is the largest absolute difference between the same oracle evaluated in float32 on the CPU and that reference: the size of
"the same arithmetic in float32", which the GPU gates are a multiple of.  It never comes from a kernel.  Every builder is seeded
and cached: a case is built once per process and must not be modified by a test."""
import functools

import numpy as np
import torch

from oracle import fixtures as FX
from oracle import geometry_oracle as G

GATE_FACTOR = 4.0  # float32 kernels: GATE_FACTOR x e32 ("the same float32 arithmetic in another order", tests/test_textenc_gpu.py)
GAP = 1e-3  # every planted minimum beats its runner-up by at least this much in float64: float32 cannot flip it

# ---- h2o / contact_min_dist ------------------------------------------------------------------------------------------------------
# (B, T, V, nobj, P, obj_num).  V walks the kernel's 4 register slots x 4 waves (v = tid + 256 i), P its 256-point LDS tile.
# Cases with V * T < 64 have a larger B: at least 64 output elements stand behind every e32.
H2O_CASES = [
    (64, 1, 1, 1, 1, None),
    (32, 2, 1, 3, 257, "ragged"),
    (3, 1, 63, 1, 255, None),
    (1, 2, 64, 3, 256, None),
    (3, 5, 64, 3, 513, [1, 3, 2]),
    (3, 2, 255, 3, 257, [3, 1, 2]),
    (1, 5, 256, 1, 513, None),
    (1, 2, 257, 1, 256, None),
    (3, 5, 257, 3, 1, [2, 3, 1]),
    (1, 2, 513, 3, 256, [2]),
    (3, 2, 769, 1, 257, None),
    (1, 2, 778, 3, 257, None),
    (3, 1, 778, 3, 255, [1, 2, 3]),
    (1, 5, 1023, 1, 257, None),
    (3, 2, 1023, 3, 256, [2, 1, 1]),
    (1, 5, 1024, 3, 513, None),
    (3, 2, 1024, 1, 1, None),
    (1, 2, 1024, 3, 257, [2]),
]
D_MIN = 1e-4  # planted frame minimum (vertex 0): the vertex sits this far from an object point
D_NEAR = 2e-3  # planted nearest point: far enough above D_MIN + GAP not to disturb a planted frame minimum
PUSH = 1.5e-3  # in the two frames with a planted minimum, other vertices closer than this are drawn again (until 4 PUSH away)


def h2o_id(c):
    B, T, V, nobj, P, on = c
    return f"B{B}-T{T}-V{V}-o{nobj}-P{P}" + ("" if on is None else "-ragged")


def _obj_num(case):
    B, _, _, nobj, _, on = case
    if on == "ragged":
        return [1 + (b * 2) % nobj for b in range(B)]
    return on


def _moved(traj64, pts64, b, o, t):
    """object o of clip b in frame t, float64 (P, 3)"""
    R = G.rot6d_to_rotmat(traj64[b, o, t, 3:9])
    return pts64[b, o] @ R.T + traj64[b, o, t, 0:3]


@functools.lru_cache(maxsize=None)
def h2o_case(i):
    """-> dict: hand (B,T,V,3), traj (B,nobj,T,9), pts (B,nobj,P,3) float32 tensors, obj_num (list or None), plants, ref (B,T,V)
    float64, e32.  plants: ("near", b, t, v, merged point index) / ("min", b, t, v) / ("contact", b, t, v)."""
    case = H2O_CASES[i]
    B, T, V, nobj, P, _ = case
    on = _obj_num(case)
    g = torch.Generator().manual_seed(1000 + i)
    hand = torch.randn(B, T, V, 3, generator=g) * 0.1
    traj = torch.randn(B, nobj, T, 9, generator=g)
    traj[..., 0:3] *= 0.05
    pts = torch.randn(B, nobj, P, 3, generator=g) * 0.1
    n_real = [nobj if on is None else int(on[b]) for b in range(B)]
    frames = [(b, t) for b in range(B) for t in range(T)]
    assert len(frames) >= 2
    # exact contact: identity pose of every real object in frame 0 of clip 0
    b0, t0 = frames[0]
    traj[b0, :, t0] = torch.tensor([0, 0, 0, 1, 0, 0, 0, 1, 0], dtype=torch.float32)
    traj64, pts64 = traj.double(), pts.double()

    def merged(b, t):
        return torch.cat([_moved(traj64, pts64, b, o, t) for o in range(n_real[b])], dim=0)

    def dist_to(b, t, x):
        return (merged(b, t) - x).norm(dim=-1)

    def unit():
        d = torch.randn(3, generator=g, dtype=torch.float64)
        return d / d.norm()

    def place(b, t, v, m, dist):
        """hand[b, t, v] = merged point m of the frame + an offset of length dist whose runner-up is clear by 2 GAP"""
        target = merged(b, t)[m]
        for _ in range(64):
            x = (target + dist * unit()).float()
            d = dist_to(b, t, x.double())
            near = d[m].item()
            d[m] = float("inf")
            if d.min().item() >= near + 2 * GAP:
                hand[b, t, v] = x
                return
        raise AssertionError(f"no clear place beside point {m} of frame {(b, t)}")

    plants = []
    # frame 0: vertex V - 1 equals an object point bit for bit (distance exactly 0: the frame minimum at v = V - 1)
    mc = (n_real[b0] - 1) * P + P // 2
    hand[b0, t0, V - 1] = pts[b0, n_real[b0] - 1, P // 2]
    plants += [("contact", b0, t0, V - 1), ("min", b0, t0, V - 1)]
    # frame 1: vertex 0 is the frame minimum
    b1, t1 = frames[1]
    place(b1, t1, 0, (7 * i) % (n_real[b1] * P), D_MIN)
    plants.append(("min", b1, t1, 0))
    for (b, t, keep) in ((b0, t0, V - 1), (b1, t1, 0)):
        d = torch.cdist(hand[b, t].double(), merged(b, t)).min(dim=-1).values  # screening only, never a reference
        for v in torch.nonzero(d < PUSH).flatten().tolist():
            while v != keep and dist_to(b, t, hand[b, t, v].double()).min().item() < 4 * PUSH:
                hand[b, t, v] = torch.randn(3, generator=g) * 0.1
    # nearest points at the ends of the point list, either side of the 256-point tile and in the last real object
    free = [v for v in range(V) if v not in (0, V - 1)]
    targets = [(0, 0), (0, P - 1), (0, 255), (0, 256), ("last", P // 2), ("last", P - 1)]
    for k, (o, j) in enumerate(targets):
        if j >= P:
            continue
        if free:
            b, t = frames[k % len(frames)]
            v = free[((k + 1) * len(free)) // (len(targets) + 1)] if k != 1 else free[-1]
        elif len(frames) > 2:
            b, t = frames[2 + k % (len(frames) - 2)]  # V <= 2: the only vertices carry the planted minima of frames 0 and 1
            v = 0
        else:
            continue
        o = n_real[b] - 1 if o == "last" else o
        if any(p[1:4] == (b, t, v) for p in plants):
            continue
        place(b, t, v, o * P + j, D_NEAR)
        plants.append(("near", b, t, v, o * P + j))
    # padded objects are poison: neither the kernel nor the reference may read them
    for b in range(B):
        traj[b, n_real[b]:] = float("nan")
        pts[b, n_real[b]:] = float("nan")
    assert mc < n_real[b0] * P
    ref = G.h2o_dist(hand.double(), traj.double(), pts.double(), on)
    e32 = float((G.h2o_dist(hand, traj, pts, on).double() - ref).abs().max())
    return dict(hand=hand, traj=traj, pts=pts, obj_num=on, n_real=n_real, plants=plants, ref=ref, e32=e32)


def h2o_frame(c, b, t):
    """float64 distances (V, n_real * P) of frame (b, t) of a built case, straight from the definition"""
    traj64, pts64 = c["traj"].double(), c["pts"].double()
    m = torch.cat([_moved(traj64, pts64, b, o, t) for o in range(c["n_real"][b])], dim=0)
    return (c["hand"][b, t].double()[:, None, :] - m[None, :, :]).norm(dim=-1)


# ---- pose decode -----------------------------------------------------------------------------------------------------------------
# (N, J): N * J on multiples of the 256-thread block (256 x 1, 256 x 2, 256 x 16) and off them
POSE_CASES = [(1, 1), (1, 16), (1, 21), (255, 1), (256, 1), (257, 1), (255, 2), (256, 2), (256, 16), (1000, 16), (257, 21),
              (1000, 21)]
POSE_SIGN_FREE = 1e-3  # rows with |w_ref| below this are compared up to sign (q and -q are the same rotation)


def quat_to_rotmat(q):
    """R(q), q = (w, x, y, z) unit, float64 (..., 3, 3)"""
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def _pose_rows(rng, n):
    """n joints: unit quaternions with w >= 0 and the rot6d (float64) whose Gram-Schmidt gives R(q) back"""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    q *= np.where(q[:, :1] < 0, -1.0, 1.0)
    if n >= 8:  # near-180-degree rotations: w = 0 exactly and w = 1e-4
        for r, w in ((1, 0.0), (2, 0.0), (3, 1e-4), (4, 1e-4)):
            xyz = q[r, 1:] / np.linalg.norm(q[r, 1:])
            q[r] = np.concatenate([[w], xyz * np.sqrt(1 - w * w)])
    R = quat_to_rotmat(q)
    s1, s2 = rng.uniform(0.5, 2.0, (n, 1)), rng.uniform(0.5, 2.0, (n, 1))
    a1 = s1 * R[:, 0]
    a2 = s2 * R[:, 1] + 0.3 * a1
    return q, np.concatenate([a1, a2], axis=-1)


def quat_err(got, ref):
    """per-row largest |difference|, float64; rows with |w_ref| < POSE_SIGN_FREE up to sign"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    e = np.abs(got - ref).max(-1)
    flip = np.abs(got + ref).max(-1)
    return np.where(np.abs(ref[..., 0]) < POSE_SIGN_FREE, np.minimum(e, flip), e)


def oracle_quat(pose, J):
    """the oracle's decode for any J (G.pose_decode itself is fixed to 16 joints): pose (N, 3 + 6J) tensor -> (N, J, 4)"""
    return G.rotmat_to_quat(G.rot6d_to_rotmat(pose[..., 3:].reshape(pose.shape[:-1] + (J, 6))))


@functools.lru_cache(maxsize=None)
def pose_case(i):
    """-> dict: pose (N, 3 + 6J) float32 tensor, quat (N, J, 4) float64 truth, e32 (this case's own), best (N, J) arg-max branch"""
    N, J = POSE_CASES[i]
    rng = np.random.default_rng(2000 + i)
    q, r6 = _pose_rows(rng, N * J)
    pose = np.concatenate([rng.normal(size=(N, 3)) * 0.3, r6.reshape(N, J * 6)], axis=-1).astype(np.float32)
    pose_t = torch.from_numpy(pose)
    q32 = oracle_quat(pose_t, J).numpy()
    q = q.reshape(N, J, 4)
    e32 = float(quat_err(q32, q).max())
    return dict(pose=pose_t, quat=q, e32=e32, best=np.argmax(np.abs(q), axis=-1), N=N, J=J)


@functools.lru_cache(maxsize=None)
def pose_e32_pooled():
    """largest float32-oracle error over every row of the table.  The rows are identically distributed, so every case's own e32
    estimates this one number; a case of fewer than 64 joints (4 to 84 outputs) estimates it badly and is gated with the pooled one."""
    return max(pose_case(i)["e32"] for i in range(len(POSE_CASES)))


def pose_gate_e32(i):
    N, J = POSE_CASES[i]
    return pose_case(i)["e32"] if N * J >= 64 else pose_e32_pooled()


DEGENERATE_KINDS = ["a1_zero", "a2_zero", "a2_parallel", "scale_1e-20", "scale_1e15"]
DEGENERATE_WELL_CONDITIONED = ["a1_zero", "a2_zero", "scale_1e15"]  # the float32 oracle is a usable reference for these


@functools.lru_cache(maxsize=None)
def pose_degenerate():
    """-> dict: pose (40, 15) float32 (J = 2; rows 8k .. 8k + 7 are of kind k), q32 the float32 oracle's answer on the CPU"""
    rng = np.random.default_rng(2999)
    _, r6 = _pose_rows(rng, 80)
    r6 = r6.reshape(5, 16, 6)
    r6[0, :, 0:3] = 0.0
    r6[1, :, 3:6] = 0.0
    r6[2, :, 3:6] = -1.7 * r6[2, :, 0:3]
    r6[3] *= 1e-20
    r6[4] *= 1e15
    pose = np.concatenate([rng.normal(size=(40, 3)), r6.reshape(40, 12)], axis=-1).astype(np.float32)
    pose_t = torch.from_numpy(pose)
    return dict(pose=pose_t, q32=oracle_quat(pose_t, 2).numpy(), kind=np.repeat(np.arange(5), 8))


# ---- transform_points ------------------------------------------------------------------------------------------------------------
# one case per P: every (T, leading shape) of it in one sweep, so that at least 96 outputs stand behind the case's e32
TRANSFORM_P = [1, 255, 256, 257, 700]
TRANSFORM_T = [1, 3]
TRANSFORM_LEAD = [(), (1,), (2, 3)]
IDENTITY_TRAJ = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


@functools.lru_cache(maxsize=None)
def transform_case(P):
    """-> dict: calls = [(traj32, pts32, ref64)] over TRANSFORM_T x TRANSFORM_LEAD (traj (..., T, 9), pts (..., P, 3) float32 tensors;
    the float64 kernel gets their .double()), e32 of the float32 oracle over all of them, cmax = largest |coordinate| of the reference"""
    g = torch.Generator().manual_seed(3000 + P)
    calls, e32, cmax = [], 0.0, 0.0
    for T in TRANSFORM_T:
        for lead in TRANSFORM_LEAD:
            traj = torch.randn(*lead, T, 9, generator=g)
            traj[..., 0:3] *= 0.05
            pts = torch.randn(*lead, P, 3, generator=g) * 0.1
            ref = G.transform_points(traj.double(), pts.double())
            e32 = max(e32, float((G.transform_points(traj, pts).double() - ref).abs().max()))
            cmax = max(cmax, float(ref.abs().max()))
            calls.append((traj, pts, ref))
    return dict(calls=calls, e32=e32, cmax=cmax)


def transform_f64_gate(cmax):
    """transform_points<double>: 64 eps64 x the largest |coordinate| (3 products and 3 sums behind an element, a normalised basis
    with a few ulp of its own), floored at 64 eps64 x 0.01"""
    return 64 * np.finfo(np.float64).eps * max(cmax, 0.01)


# ---- vertex normals --------------------------------------------------------------------------------------------------------------
NORMALS_V = [3, 4, 255, 256, 257]
NORMALS_M = [1, 2, 331]  # n_mesh * V: 3 ... 85 067, on and off multiples of the 256-thread block
NORMALS_CASES = [(V, M) for V in NORMALS_V for M in NORMALS_M]


@functools.lru_cache(maxsize=None)
def normals_case(V, M):
    """-> dict: verts (M, V, 3) float32 numpy (the last mesh scaled by 1e-3: |n| < 1e-6), faces (F, 3) int64 with unreferenced
    vertices, one zero-area face and one duplicated face, unref (vertex ids without a face), ref32 the float32 oracle's normals"""
    rng = np.random.default_rng(4000 + 7 * V + M)
    n_unref = 0 if V == 3 else 1 if V == 4 else 5  # (three vertices are one triangle: nothing to leave out)
    used = np.sort(rng.permutation(V)[: V - n_unref])
    Fn = max(2, 2 * V)
    faces = np.stack([rng.permutation(used)[:3] for _ in range(Fn)]).astype(np.int64)
    faces[Fn // 2] = faces[0]  # a duplicated face
    faces[-1] = [faces[-1][0], faces[-1][1], faces[-1][0]]  # a zero-area face
    unref = np.setdiff1d(np.arange(V), faces.reshape(-1))
    verts = (rng.normal(size=(M, V, 3)) * 0.1).astype(np.float32)
    verts[-1] *= np.float32(1e-3)
    return dict(verts=verts, faces=faces, unref=unref, ref32=G.vertex_normals(verts, faces))


def normals_definition_f64(verts, faces):
    """the definition in float64: (n (M, V, 3) normalised with x / max(|x|, 1e-6), |sum| (M, V), sum of |a| |b| over a vertex's
    corners (M, V) - the size of the terms whose rounding the float32 sum carries)"""
    x = np.asarray(verts, np.float64)
    n = np.zeros_like(x)
    mag = np.zeros(x.shape[:2])
    for c in range(3):
        v, a, b = faces[:, c], faces[:, (c + 1) % 3], faces[:, (c + 2) % 3]
        ea, eb = x[:, a] - x[:, v], x[:, b] - x[:, v]
        for m in range(x.shape[0]):
            np.add.at(n[m], v, np.cross(ea[m], eb[m]))
            np.add.at(mag[m], v, np.linalg.norm(ea[m], axis=-1) * np.linalg.norm(eb[m], axis=-1))
    ln = np.linalg.norm(n, axis=-1)
    return n / np.maximum(ln, 1e-6)[..., None], ln, mag


# ---- mesh_contains ---------------------------------------------------------------------------------------------------------------
CONTAINS_MESHES = [(0, 64), (0, 65), (1, 128), (1, 129)]  # (icosphere subdivisions, F after padding): the 64-triangle LDS tile
CONTAINS_N = [1, 255, 256, 257]  # the 256-point block
RESOLUTION = 512


@functools.lru_cache(maxsize=None)
def contains_mesh(subdiv, F):
    v, f = FX.icosphere(subdiv)
    pad = np.arange(F - len(f), dtype=np.int64) % len(v)
    return v, np.concatenate([f, np.stack([pad, pad, pad], axis=1)], axis=0)


def _rescale(v, f):
    tri = v[f].reshape(-1, 3)
    bmin, bmax = tri.min(axis=0), tri.max(axis=0)
    scale = (RESOLUTION - 1) / (bmax - bmin)
    return bmin, bmax, scale, 0.5 - scale * bmin


def _hits_resolution(scale, translate, axis):
    """a coordinate whose rescaled value scale * x + translate is exactly RESOLUTION in float64"""
    x = (RESOLUTION - translate[axis]) / scale[axis]
    for _ in range(64):
        y = scale[axis] * x + translate[axis]
        if y == RESOLUTION:
            return x
        x = np.nextafter(x, np.inf if y < RESOLUTION else -np.inf)
    raise AssertionError("no float64 lands on the resolution")


@functools.lru_cache(maxsize=None)
def contains_case(subdiv, F, N):
    """-> dict: verts, faces, points (N + extras, 3) float64 (the first N inside the bounding box), ref bool, n_box = N,
    at_res = rows whose rescaled coordinate is exactly RESOLUTION (axis = row - first of them)"""
    v, f = contains_mesh(subdiv, F)
    bmin, bmax, scale, translate = _rescale(v, f)
    rng = np.random.default_rng(5000 + 10 * F + N)
    box = bmin + rng.random((N, 3)) * (bmax - bmin)
    extra = []
    for ax in range(3):
        for lim, out in ((bmin, -1.0), (bmax, 1.0)):
            on = bmin + rng.random(3) * (bmax - bmin)
            on[ax] = lim[ax]  # exactly on a bounding-box face
            off = on.copy()
            off[ax] = np.nextafter(lim[ax], out * np.inf)  # one ulp outside it
            far = on.copy()
            far[ax] = lim[ax] + out * 0.6 / scale[ax]  # past the half-cell margin of the rescaled frame
            extra += [on, off, far]
    first_res = N + len(extra)
    for ax in range(3):
        p = bmin + 0.5 * (bmax - bmin)  # the centre, moved along one axis to the rescaled coordinate `resolution`
        p[ax] = _hits_resolution(scale, translate, ax)
        extra.append(p)
    pts = np.concatenate([box, np.asarray(extra)], axis=0)
    return dict(verts=v, faces=f, points=pts, ref=G.mesh_contains(v, f, pts, RESOLUTION), n_box=N,
                at_res=list(range(first_res, first_res + 3)), scale=scale, translate=translate)
