"""Native MANO hand layer: `HipManoLayer` runs the MANO forward kinematics and linear blend skinning on the HIP kernel of
libtamf_mano.so (include/tamf_mano.h, csrc/tamf_mano.h), with the call contract the launchers and SegmentRefineModel use for their
MANO layers: `layer(pose_coeffs=(N, 16, 4) quaternions, betas=(N, 10)) -> .verts (N, V, 3), .joints (N, 21, 3)`, `.th_faces`,
`.get_mano_closed_faces()`.

The MANO assets are licence-gated and not part of this package: the model arrays come from the user (`ManoArrays.from_npz`, files
written by tools/mano_pkl_to_npz.py from the user's own MANO_RIGHT.pkl / MANO_LEFT.pkl).  The arrays are used as given; any sign fix
of the left hand's shape basis is the converter's (the user's) business, not this layer's.

What is implemented is the published definition (SMPL, Loper et al. 2015; MANO, Romero et al. 2017) in the configuration of the
reference's call sites: `ManoLayer(rot_mode="quat", center_idx=0, use_pca=False, flat_hand_mean=True)`.  It is pinned on analytic cases and on a
float64 restatement of the definition (tests/mano_restatement.py); parity with the manotorch package itself is NOT verified - its
source was not available.  Every convention that cannot be derived from the call sites is a parameter with manopth's published
default: the fingertip vertex ids, the 21-joint order, the centre joint.  The wrist cap of `close_wrist` is this package's own
triangulation and may differ from manotorch's closed faces; it matters only to the SIV score's containment test near the wrist.

Autograd: `HipManoLayer(..., differentiable=True)` (factory: `make_mano_differentiable`) runs the call through a
`torch.autograd.Function` whose backward is tamf_mano_backward, the HIP vector-Jacobian product of the same function - gradients with
respect to the quaternions (as given: the normalisation is differentiated too) and the betas, none with respect to the model arrays,
no double backward.  The default layer stays inference only and refuses an input that requires grad.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p
from typing import Optional

import numpy as np

N_JOINTS, N_BETAS, N_POSE, N_TIPS, N_OUT_JOINTS, V_MAX = 16, 10, 135, 5, 21, 1024
DEFAULT_TIP_IDS = (745, 317, 444, 556, 673)  # manopth: thumb, index, middle, ring, pinky
DEFAULT_JOINT_ORDER = (0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20)  # over (16 chain joints | 5 tips)


def _float_array(name, a, shape):
    a = np.asarray(a)
    if a.dtype.kind != "f":
        raise TypeError(f"{name}: expected a floating-point array, got {a.dtype}")
    if a.shape != shape:
        raise ValueError(f"{name}: expected shape {shape}, got {a.shape}")
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError(f"{name}: holds a non-finite value")
    return a


def _int_array(name, a, shape, lo, hi):
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{name}: expected an integer array, got {a.dtype}")
    if len(shape) != a.ndim or any(s is not None and s != t for s, t in zip(shape, a.shape)):
        raise ValueError(f"{name}: expected shape {shape}, got {a.shape}")
    a = np.ascontiguousarray(a, dtype=np.int64)
    if a.size and (a.min() < lo or a.max() >= hi):
        raise ValueError(f"{name}: values outside [{lo}, {hi})")
    return a


class ManoArrays:
    """The arrays of one MANO hand model, validated: v_template (V,3), shapedirs (V,3,10), posedirs (V,3,135), J_regressor (16,V),
    weights (V,16) - float, kept as float64 -, parents (16,) int with the root first (parents[0] < 0 or any value: it is stored as
    -1) and every other parent below its child, faces (F,3) int; optional closed_faces (F',3), tip_ids (5,), joint_order (21,)."""

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, weights, parents, faces, closed_faces=None, tip_ids=None,
                 joint_order=None):
        vt = np.asarray(v_template)
        if vt.ndim != 2 or vt.shape[1] != 3 or not 1 <= vt.shape[0] <= V_MAX:
            raise ValueError(f"v_template: expected shape (V, 3) with 1 <= V <= {V_MAX}, got {vt.shape}")
        V = int(vt.shape[0])
        self.v_template = _float_array("v_template", vt, (V, 3))
        self.shapedirs = _float_array("shapedirs", shapedirs, (V, 3, N_BETAS))
        self.posedirs = _float_array("posedirs", posedirs, (V, 3, N_POSE))
        self.J_regressor = _float_array("J_regressor", J_regressor, (N_JOINTS, V))
        self.weights = _float_array("weights", weights, (V, N_JOINTS))
        par = np.asarray(parents)
        if par.dtype.kind not in "iu" or par.shape != (N_JOINTS,):
            raise ValueError(f"parents: expected {N_JOINTS} integers, got {par.dtype} {par.shape}")
        par = par.astype(np.int64)
        # (a pickle's kintree_table holds 2**32 - 1 for the root)
        if 0 <= par[0] < N_JOINTS:
            raise ValueError("parents: joint 0 must be the root (parents[0] = -1)")
        par[0] = -1
        for j in range(1, N_JOINTS):
            if not 0 <= par[j] < j:
                raise ValueError(f"parents[{j}] = {par[j]}: not a tree with root 0 and every parent index below its child")
        self.parents = par
        self.faces = _int_array("faces", faces, (None, 3), 0, V)
        self.closed_faces = None if closed_faces is None else _int_array("closed_faces", closed_faces, (None, 3), 0, V)
        self.tip_ids = _int_array("tip_ids", DEFAULT_TIP_IDS if tip_ids is None else tip_ids, (N_TIPS,), 0, V)
        self.joint_order = _int_array("joint_order", DEFAULT_JOINT_ORDER if joint_order is None else joint_order, (N_OUT_JOINTS,), 0,
                                      N_OUT_JOINTS)
        if sorted(self.joint_order.tolist()) != list(range(N_OUT_JOINTS)):
            raise ValueError("joint_order: not a permutation of 0..20")

    @property
    def n_verts(self) -> int:
        return int(self.v_template.shape[0])

    FIELDS = ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "parents", "faces")
    OPTIONAL = ("closed_faces", "tip_ids", "joint_order")

    @classmethod
    def from_npz(cls, path) -> "ManoArrays":
        """the .npz tools/mano_pkl_to_npz.py writes (FIELDS, and any of OPTIONAL)"""
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in cls.FIELDS if k not in z.files]
            if missing:
                raise KeyError(f"{path}: missing arrays {missing}")
            return cls(**{k: z[k] for k in cls.FIELDS + cls.OPTIONAL if k in z.files})

    def to_npz(self, path) -> None:
        d = {k: getattr(self, k) for k in self.FIELDS + self.OPTIONAL if getattr(self, k) is not None}
        np.savez(path, **d)


def close_wrist(faces) -> np.ndarray:
    """faces (F,3) of an open, consistently oriented mesh with ONE hole -> (F + L - 2, 3): the faces plus a cap over the hole.
    The boundary (the directed edges whose reverse is in no face) must be one simple loop of L vertices; anything else raises
    ValueError.  The loop is walked against the direction of its adjacent faces, so the cap is oriented like the mesh, and is
    triangulated as a fan from the loop vertex with the lowest index; no vertex is added.  These cap triangles are this package's own
    and may differ from manotorch's `get_mano_closed_faces()`."""
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu":
        raise ValueError(f"faces: expected an integer (F, 3) array, got {f.dtype} {f.shape}")
    f = f.astype(np.int64)
    directed = {}
    for a, b, c in f.tolist():
        for e in ((a, b), (b, c), (c, a)):
            if e[0] == e[1] or e in directed:
                raise ValueError(f"faces: directed edge {e} is degenerate or used by two faces (not consistently oriented)")
            directed[e] = True
    boundary = [e for e in directed if (e[1], e[0]) not in directed]
    if len(boundary) < 3:
        raise ValueError("faces: the mesh has no hole to close")
    # against the faces: the cap's edge is the reverse (b, a) of a boundary edge (a, b)
    nxt = {}
    for a, b in boundary:
        if b in nxt:
            raise ValueError(f"faces: boundary vertex {b} lies on more than one boundary edge (the boundary is not a simple loop)")
        nxt[b] = a
    start = min(nxt)
    loop, v = [start], nxt[start]
    while v != start:
        if v not in nxt or len(loop) > len(nxt):
            raise ValueError("faces: the boundary is not a closed loop")
        loop.append(v)
        v = nxt[v]
    if len(loop) != len(nxt):
        raise ValueError(f"faces: the boundary has more than one loop ({len(nxt)} boundary edges, {len(loop)} on the first loop)")
    cap = np.array([[loop[0], loop[i], loop[i + 1]] for i in range(1, len(loop) - 1)], dtype=np.int64)
    return np.concatenate([f, cap], axis=0)


class ManoOutput:
    """what a layer call returns: verts (N, V, 3), joints (N, 21, 3) - float32 tensors on the layer's device"""
    __slots__ = ("verts", "joints")

    def __init__(self, verts, joints):
        self.verts, self.joints = verts, joints


_bound = None


def _bind():
    global _bound
    if _bound is None:
        from . import _lib

        lib = _lib.load_mano_lib()
        lib.tamf_mano_last_error.restype = ctypes.c_char_p
        lib.tamf_mano_model_create.argtypes = [c_int32] + [POINTER(c_double)] * 5 + [POINTER(c_int32)] * 3 + [c_int32, POINTER(c_void_p)]
        lib.tamf_mano_model_destroy.argtypes = [c_void_p]
        lib.tamf_mano_model_set_tiles.argtypes = [c_void_p, c_int32]
        lib.tamf_mano_forward.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]
        lib.tamf_mano_backward.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        _bound = lib
    return _bound


def _check(lib, rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"libtamf_mano: {lib.tamf_mano_last_error().decode()} (status {rc})")


def _aligned16(t):
    """the kernels read a frame's quaternions as float4: a contiguous view that starts off a 16-byte boundary is copied"""
    return t.clone() if t.data_ptr() % 16 else t


_function = None


def _mano_function():
    """the torch.autograd.Function of a differentiable layer (built on first use: torch is imported lazily in this module)"""
    global _function
    if _function is None:
        import torch

        class ManoFunction(torch.autograd.Function):
            @staticmethod
            def forward(ctx, layer, q, b, with_joints):
                verts, joints = layer._run_forward(q, b, with_joints)
                ctx.layer = layer
                ctx.save_for_backward(q, b)
                ctx.set_materialize_grads(False)  # an output nothing depends on arrives as None and is passed as NULL
                if joints is None:
                    return verts
                return verts, joints

            @staticmethod
            def backward(ctx, dverts, djoints=None):
                if torch.is_grad_enabled():  # (a backward that is itself recorded: create_graph=True)
                    raise RuntimeError("HipManoLayer: double backward is not supported (the HIP backward is first order only; "
                                       "call backward / autograd.grad without create_graph)")
                if dverts is None and djoints is None:
                    return None, None, None, None
                q, b = ctx.saved_tensors
                dq, db = ctx.layer.backward_raw(q, b, dverts, djoints, want_dbetas=ctx.needs_input_grad[2])
                return None, dq if ctx.needs_input_grad[1] else None, db, None

        _function = ManoFunction
    return _function


class HipManoLayer:
    """MANO forward on the GPU for one hand model.  `center_idx`: the OUTPUT joint subtracted from vertices and joints (0: the wrist,
    as the reference's layers are built), or None.  A missing kernel library or a device that is no GPU is an error; there is no
    torch fall-back.  `differentiable`: False (the default) is the inference layer, which refuses an input that requires grad; True
    carries autograd through the call with the HIP backward (first order only: a double backward raises)."""

    def __init__(self, arrays: ManoArrays, center_idx: Optional[int] = 0, device="cuda", differentiable: bool = False):
        import torch

        from .hip_backend import require_gpu

        if not isinstance(arrays, ManoArrays):
            raise TypeError("arrays must be a ManoArrays")
        if center_idx is not None and not 0 <= int(center_idx) < N_OUT_JOINTS:
            raise ValueError(f"center_idx = {center_idx} outside [0, {N_OUT_JOINTS})")
        self.device = require_gpu(torch.device(device))
        self.arrays, self.center_idx = arrays, None if center_idx is None else int(center_idx)
        self.differentiable = bool(differentiable)
        self._lib = _bind()
        self._model = c_void_p()

        def dp(a):
            return a.ctypes.data_as(POINTER(c_double))

        def ip(a):
            return np.ascontiguousarray(a, dtype=np.int32)

        par, tips, order = ip(arrays.parents), ip(arrays.tip_ids), ip(arrays.joint_order)
        with torch.cuda.device(self.device):
            _check(self._lib, self._lib.tamf_mano_model_create(
                arrays.n_verts, dp(arrays.v_template), dp(arrays.shapedirs), dp(arrays.posedirs), dp(arrays.J_regressor),
                dp(arrays.weights), par.ctypes.data_as(POINTER(c_int32)), tips.ctypes.data_as(POINTER(c_int32)),
                order.ctypes.data_as(POINTER(c_int32)), -1 if self.center_idx is None else self.center_idx, ctypes.byref(self._model)))
        self.th_faces = torch.from_numpy(arrays.faces).long().to(self.device)
        self._closed = None

    def set_tiles(self, m_tiles: int) -> None:
        """tuning only (tools/mano_bench.py): 16-frame tiles per workgroup, 1 / 2 / 4, 0 = built-in choice; no output bit changes"""
        _check(self._lib, self._lib.tamf_mano_model_set_tiles(self._model, int(m_tiles)))

    def get_mano_closed_faces(self):
        """the asset's closed faces when it has them, else close_wrist(faces); a LongTensor on the layer's device"""
        import torch

        if self._closed is None:
            cf = self.arrays.closed_faces if self.arrays.closed_faces is not None else close_wrist(self.arrays.faces)
            self._closed = torch.from_numpy(np.ascontiguousarray(cf)).long().to(self.device)
        return self._closed

    def forward(self, pose_coeffs, betas, with_joints: bool = True) -> ManoOutput:
        import torch

        from .hip_backend import _stream_ptr

        if not isinstance(pose_coeffs, torch.Tensor) or not isinstance(betas, torch.Tensor):
            raise TypeError("pose_coeffs and betas must be torch tensors")
        needs_grad = torch.is_grad_enabled() and (pose_coeffs.requires_grad or betas.requires_grad)
        if not self.differentiable and (pose_coeffs.requires_grad or betas.requires_grad):
            raise RuntimeError("HipManoLayer is inference only: an input requires grad (build the layer with differentiable=True)")
        if pose_coeffs.dim() != 3 or tuple(pose_coeffs.shape[1:]) != (N_JOINTS, 4):
            raise ValueError(f"pose_coeffs: expected (N, 16, 4) quaternions, got {tuple(pose_coeffs.shape)}")
        N = int(pose_coeffs.shape[0])
        if tuple(betas.shape) != (N, N_BETAS):
            raise ValueError(f"betas: expected ({N}, {N_BETAS}), got {tuple(betas.shape)}")
        if self._model is None or not self._model.value:
            raise RuntimeError("HipManoLayer is closed")
        if needs_grad:
            # (the conversions stay in the graph; the Function sees float32 contiguous tensors on the layer's device)
            q = pose_coeffs.to(device=self.device, dtype=torch.float32).contiguous()
            b = betas.to(device=self.device, dtype=torch.float32).contiguous()
            out = _mano_function().apply(self, q, b, bool(with_joints))
            return ManoOutput(*out) if with_joints else ManoOutput(out, None)
        q = pose_coeffs.detach().to(device=self.device, dtype=torch.float32).contiguous()
        b = betas.detach().to(device=self.device, dtype=torch.float32).contiguous()
        return ManoOutput(*self._run_forward(q, b, with_joints))

    def _run_forward(self, q, b, with_joints: bool):
        """tamf_mano_forward on float32 contiguous device tensors -> (verts, joints or None)"""
        import torch

        from .hip_backend import _stream_ptr

        N, V = int(q.shape[0]), self.arrays.n_verts
        q = _aligned16(q)
        verts = torch.empty((N, V, 3), dtype=torch.float32, device=self.device)
        joints = torch.empty((N, N_OUT_JOINTS, 3), dtype=torch.float32, device=self.device) if with_joints else None
        if N > 0:
            with torch.cuda.device(self.device):
                _check(self._lib, self._lib.tamf_mano_forward(self._model, q.data_ptr(), b.data_ptr(), N, verts.data_ptr(),
                                                             joints.data_ptr() if with_joints else None, _stream_ptr(self.device)))
        return verts, joints

    def backward_raw(self, pose_coeffs, betas, dverts=None, djoints=None, want_dbetas: bool = True):
        """tamf_mano_backward: the gradients (dquat (N, 16, 4), dbetas (N, 10) or None) of the layer's outputs' upstream gradients
        `dverts` (N, V, 3) / `djoints` (N, 21, 3) - either may be None (zeros), not both.  Recomputes what it needs from the inputs;
        no forward call has to precede it.  N = 0 returns empty gradients without a launch."""
        import torch

        from .hip_backend import _stream_ptr

        if self._model is None or not self._model.value:
            raise RuntimeError("HipManoLayer is closed")
        N, V = int(pose_coeffs.shape[0]), self.arrays.n_verts
        if tuple(pose_coeffs.shape) != (N, N_JOINTS, 4) or tuple(betas.shape) != (N, N_BETAS):
            raise ValueError(f"expected quaternions (N, 16, 4) and betas (N, 10), got {tuple(pose_coeffs.shape)} and {tuple(betas.shape)}")

        def f32(t, shape, name):
            if t is None:
                return None
            if tuple(t.shape) != shape:
                raise ValueError(f"{name}: expected {shape}, got {tuple(t.shape)}")
            return t.detach().to(device=self.device, dtype=torch.float32).contiguous()

        q, b = _aligned16(f32(pose_coeffs, (N, N_JOINTS, 4), "pose_coeffs")), f32(betas, (N, N_BETAS), "betas")
        dv, dj = f32(dverts, (N, V, 3), "dverts"), f32(djoints, (N, N_OUT_JOINTS, 3), "djoints")
        dq = torch.empty((N, N_JOINTS, 4), dtype=torch.float32, device=self.device)
        db = torch.empty((N, N_BETAS), dtype=torch.float32, device=self.device) if want_dbetas else None
        if N > 0:
            with torch.cuda.device(self.device):
                _check(self._lib, self._lib.tamf_mano_backward(self._model, q.data_ptr(), b.data_ptr(), N, None if dv is None else dv.data_ptr(),
                                                              None if dj is None else dj.data_ptr(), dq.data_ptr(),
                                                              None if db is None else db.data_ptr(), _stream_ptr(self.device)))
        return dq, db

    __call__ = forward

    def close(self) -> None:
        """frees the device arrays (after the device has finished the layer's work)"""
        if getattr(self, "_model", None) is not None and self._model.value:
            import torch

            torch.cuda.synchronize(self.device)
            self._lib.tamf_mano_model_destroy(self._model)
            self._model = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _make_layers(mano_cfg, device, who, **layer_kw):
    d = mano_cfg.get("mano_path")
    if not d:
        raise SystemExit(f"{who}: --mano.mano_path DIR (holding MANO_RIGHT.npz and MANO_LEFT.npz) is required")
    paths = [os.path.join(str(d), n) for n in ("MANO_RIGHT.npz", "MANO_LEFT.npz")]
    for p in paths:
        if not os.path.exists(p):
            raise SystemExit(f"{who}: {p} not found; convert your MANO_RIGHT.pkl / MANO_LEFT.pkl with tools/mano_pkl_to_npz.py "
                             "(the MANO assets are licence-gated and not shipped)")
    arrays = [ManoArrays.from_npz(p) for p in paths]
    layers = [HipManoLayer(a, center_idx=0, device=device, **layer_kw) for a in arrays]
    closed = [l.get_mano_closed_faces().cpu().numpy() for l in layers]
    return layers[0], layers[1], closed[0], closed[1]


def make_mano(mano_cfg, device):
    """`--mano.factory oakink2_tamf_amd.mano:make_mano --mano.mano_path DIR`: DIR/MANO_RIGHT.npz and DIR/MANO_LEFT.npz (written by
    tools/mano_pkl_to_npz.py) -> (layer_rh, layer_lh, closed_faces_rh, closed_faces_lh), the tuple launch/sample_refine.py:load_mano
    documents; the layers are centred on joint 0 as the reference's are."""
    return _make_layers(mano_cfg, device, "make_mano")


def make_mano_differentiable(mano_cfg, device):
    """make_mano with `differentiable=True` layers: what a trainer's reconstruction losses (model/reconstruction_loss.py) need"""
    return _make_layers(mano_cfg, device, "make_mano_differentiable", differentiable=True)


__all__ = ["ManoArrays", "HipManoLayer", "ManoOutput", "close_wrist", "make_mano", "make_mano_differentiable", "DEFAULT_TIP_IDS", "DEFAULT_JOINT_ORDER"]
