"""Native object embeddings: `HipPointEncoder` runs the PointBERT point encoder (reference model/pointbert/point_encoder.py
`PointTransformer` with dvae.py `Group` / `Encoder` and misc.py `fps`) on the HIP kernels of libtamf_pointenc.so
(include/tamf_pointenc.h, csrc/tamf_pointenc.h): a point cloud (N, 3 or 6) -> the 768-vector `obj_embedding` that the denoiser, the
refiner and the FID encoder condition on.  Eval mode, float32, inference only.

The weights are not part of this package (the reference ships none either): `load_checkpoint` takes a checkpoint whose
`ckpt['state_dict']` holds the encoder under `module.point_encoder.`, as `PointTransformer.load_checkpoint` does.  Parity with the
reference is pinned on seeded weights (tests/test_pointenc_gpu.py against tools/capture_pointenc_golden.py).  How the published
embeddings were preprocessed - colour channels, normalisation, the FPS start - is not stated by the reference, so reproducing the
published `.pt` files is not verified.

The reference draws the FPS start index with `torch.randint`; here it is an argument (`start_index`, or `seed` for a draw from a CPU
generator; default: index 0), so an embedding is a function of the cloud, the weights and that index."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_float, c_int32, c_int64, c_void_p
from typing import Dict, List, Mapping, Optional, Tuple

import numpy as np

from ._native import NativeLibrary, NativeModel

PREFIX = "module.point_encoder."
# PointTransformer_8192point_2layer.yaml as model/pointbert/cfg.py:load_cfg switches it (point_dims 6, use_max_pool)
DEFAULT_CFG = dict(point_dims=6, trans_dim=384, depth=12, num_heads=6, num_group=512, group_size=32, encoder_dims=256, npoints=8192)
CFG_FIELDS = ("point_dims", "trans_dim", "depth", "num_heads", "num_group", "group_size", "encoder_dims")
N_MAX = 32768
MAX_CLOUDS_PER_CALL = 4  # bounds the workspace (87 MB per full-size cloud); no output bit depends on it


class _Config(ctypes.Structure):
    _fields_ = [(k, c_int32) for k in CFG_FIELDS]


def make_cfg(cfg: Optional[Mapping] = None) -> Dict[str, int]:
    """DEFAULT_CFG overridden by `cfg` (unknown fields are an error; the yaml's fields this encoder does not use are accepted)"""
    ignored = ("NAME", "drop_path_rate", "cls_dim", "projection_hidden_layer", "projection_hidden_dim", "use_max_pool")
    out = dict(DEFAULT_CFG)
    for k, v in dict(cfg or {}).items():
        if k in ignored:
            continue
        if k not in out:
            raise KeyError(f"point encoder cfg: unknown field {k!r} (known: {sorted(out)})")
        out[k] = int(v)
    return out


def expected_shapes(cfg: Mapping[str, int]) -> Dict[str, Tuple[int, ...]]:
    """state-dict name (without PREFIX) -> shape, in the reference module's order; BatchNorm's num_batches_tracked is no weight"""
    C, D, E = int(cfg["point_dims"]), int(cfg["trans_dim"]), int(cfg["encoder_dims"])
    s: Dict[str, Tuple[int, ...]] = {}
    for p, in0, mid, out in (("encoder.first_conv.", C, 128, 256), ("encoder.second_conv.", 512, 512, E)):
        s[p + "0.weight"], s[p + "0.bias"] = (mid, in0, 1), (mid,)
        for n in ("weight", "bias", "running_mean", "running_var"):
            s[p + "1." + n] = (mid,)
        s[p + "3.weight"], s[p + "3.bias"] = (out, mid, 1), (out,)
    s["reduce_dim.weight"], s["reduce_dim.bias"] = (D, E), (D,)
    s["cls_token"], s["cls_pos"] = (1, 1, D), (1, 1, D)
    s["pos_embed.0.weight"], s["pos_embed.0.bias"] = (128, 3), (128,)
    s["pos_embed.2.weight"], s["pos_embed.2.bias"] = (D, 128), (D,)
    for l in range(int(cfg["depth"])):
        p = f"blocks.blocks.{l}."
        s[p + "norm1.weight"], s[p + "norm1.bias"] = (D,), (D,)
        s[p + "norm2.weight"], s[p + "norm2.bias"] = (D,), (D,)
        s[p + "mlp.fc1.weight"], s[p + "mlp.fc1.bias"] = (4 * D, D), (4 * D,)
        s[p + "mlp.fc2.weight"], s[p + "mlp.fc2.bias"] = (D, 4 * D), (D,)
        s[p + "attn.qkv.weight"] = (3 * D, D)
        s[p + "attn.proj.weight"], s[p + "attn.proj.bias"] = (D, D), (D,)
    s["norm.weight"], s["norm.bias"] = (D,), (D,)
    return s


def map_checkpoint(state_dict: Mapping, cfg: Mapping[str, int]):
    """The encoder's tensors out of a checkpoint's state dict, as PointTransformer.load_checkpoint selects them: keys under
    `module.point_encoder.` with the prefix removed, everything else dropped.  -> (tensors, missing, unexpected): `missing` the
    encoder's names the checkpoint lacks, `unexpected` the prefixed names the encoder does not have (BatchNorm's
    num_batches_tracked counters are not reported: they are no weights)."""
    want = expected_shapes(cfg)
    got = {k[len(PREFIX):]: v for k, v in state_dict.items() if k.startswith(PREFIX)}
    missing = [k for k in want if k not in got]
    unexpected = [k for k in got if k not in want and not k.endswith(".num_batches_tracked")]
    return {k: got[k] for k in want if k in got}, missing, unexpected


class PointEncoderError(RuntimeError):
    pass


def _argtypes(lib) -> None:
    lib.tamf_pointenc_finalize.argtypes = [c_void_p]
    lib.tamf_pointenc_fold_bn.argtypes = [POINTER(c_float)] * 6 + [c_int32] * 3 + [POINTER(c_float)] * 2
    lib.tamf_pointenc_fps.argtypes = [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]
    lib.tamf_pointenc_group.argtypes = [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]
    lib.tamf_pointenc_workspace_bytes.argtypes = [c_void_p, c_int32]
    lib.tamf_pointenc_encode.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p]


_NATIVE = NativeLibrary("pointenc", PointEncoderError, _argtypes)
_bind, _check = _NATIVE.bind, _NATIVE.check


def fold_bn(w, b, gamma, beta, running_mean, running_var, ld_out: Optional[int] = None):
    """tamf_pointenc_fold_bn on host arrays (no GPU involved): w (out, in) float32 and the five (out,) vectors ->
    (w_folded (out, ld_out), b_folded (out,)) float32, composed in float64 by the library."""
    lib = _bind()
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(np.shape(w)[0], -1))
    vec = [np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1)) for v in (b, gamma, beta, running_mean, running_var)]
    out_ch, in_ch = w.shape
    if any(v.shape != (out_ch,) for v in vec):
        raise ValueError(f"fold_bn: every vector must have {out_ch} entries")
    ld = in_ch if ld_out is None else int(ld_out)
    wo, bo = np.empty((out_ch, ld), np.float32), np.empty((out_ch,), np.float32)

    def fp(a):
        return a.ctypes.data_as(POINTER(c_float))

    _check(lib.tamf_pointenc_fold_bn(fp(w), *[fp(v) for v in vec], out_ch, in_ch, ld, fp(wo), fp(bo)))
    return wo, bo


def fps_indices(points, num: int, start_index: int = 0):
    """tamf_pointenc_fps without a model (no weights, no cfg): one cloud `points` (N, >= 3), a float32 tensor on a GPU ->
    `num` indices (int64, on that device), [0] = start_index.  The entry point, distance and tie rule of HipPointEncoder.fps."""
    import torch

    from ..hip_backend import _stream_ptr, require_gpu

    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] < 3 or points.dtype != torch.float32:
        raise ValueError("fps_indices: expected a float32 tensor of shape (N, >= 3)")
    device = require_gpu(points.device)
    N, C = int(points.shape[0]), int(points.shape[1])
    if not 1 <= N <= N_MAX:
        raise ValueError(f"fps_indices: {N} points, the FPS kernel takes 1..{N_MAX}")
    if not 1 <= int(num) <= N or not 0 <= int(start_index) < N:
        raise ValueError(f"fps_indices: cannot sample {num} of {N} points from index {start_index}")
    lib = _bind()
    p = points.detach().contiguous()
    start = torch.full((1,), int(start_index), dtype=torch.int32, device=device)
    out = torch.empty((1, int(num)), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _check(lib.tamf_pointenc_fps(p.data_ptr(), start.data_ptr(), 1, N, C, int(num), out.data_ptr(), _stream_ptr(device)))
    return out[0].long()


class HipPointEncoder(NativeModel):
    """The point encoder on the GPU.  `cfg`: the fields of DEFAULT_CFG (missing ones take their defaults).  A missing kernel library
    or a device that is no GPU is an error; there is no torch fall-back."""

    _native = _NATIVE

    def __init__(self, cfg: Optional[Mapping] = None, device="cuda"):
        import torch

        from ..hip_backend import require_gpu

        self.cfg = make_cfg(cfg)
        self.device = require_gpu(torch.device(device))
        self._lib = _bind()
        self._model = c_void_p()
        self._loaded = False
        c = _Config(**{k: self.cfg[k] for k in CFG_FIELDS})
        _check(self._lib.tamf_pointenc_model_create(ctypes.byref(c), ctypes.byref(self._model)))

    @property
    def out_dim(self) -> int:
        return 2 * self.cfg["trans_dim"]

    # ---- weights ----
    def load_state_dict(self, state_dict: Mapping) -> None:
        """names without the `module.point_encoder.` prefix -> tensors / arrays.  A missing name, a wrong shape, an unknown name or a
        non-finite value raises PointEncoderError (num_batches_tracked counters are skipped)."""
        if self._loaded:
            raise PointEncoderError("the weights are loaded already")
        self._load_weights({k: v for k, v in state_dict.items() if not k.endswith(".num_batches_tracked")})
        self._loaded = True

    def load_checkpoint(self, path) -> Tuple[List[str], List[str]]:
        """A checkpoint with ckpt['state_dict'] holding the encoder under `module.point_encoder.` (what
        PointTransformer.load_checkpoint reads).  -> (missing, unexpected); missing names are an error here, unexpected ones are
        reported and ignored."""
        import logging

        import torch

        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(ckpt, Mapping) or "state_dict" not in ckpt:
            raise PointEncoderError(f"{path}: no 'state_dict' entry")
        sd, missing, unexpected = map_checkpoint(ckpt["state_dict"], self.cfg)
        log = logging.getLogger(__name__)
        if unexpected:
            log.warning("point encoder: unexpected keys in %s: %s", path, unexpected)
        if missing:
            raise PointEncoderError(f"{path}: missing keys {missing}")
        self.load_state_dict(sd)
        log.info("point encoder: weights loaded from %s", path)
        return missing, unexpected

    # ---- stages ----
    def _points(self, points, channels: Optional[int] = None):
        import torch

        p = torch.as_tensor(points)
        if p.dim() == 2:
            p = p[None]
        if p.dim() != 3 or p.shape[2] < 3 or (channels is not None and p.shape[2] != channels):
            raise ValueError(f"points: expected (B, N, {channels if channels else '>= 3'}), got {tuple(p.shape)}")
        if not 1 <= p.shape[1] <= N_MAX or p.shape[0] < 1:
            raise ValueError(f"points: need at least one cloud of 1..{N_MAX} points, got {tuple(p.shape)}")
        p = p.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if not bool(torch.isfinite(p).all()):
            raise ValueError("points: holds a non-finite value")
        return p

    def _indices(self, name, idx, shape, n):
        import torch

        t = torch.as_tensor(idx).to(self.device)
        if t.dtype.is_floating_point or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected integers of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
            raise ValueError(f"{name}: values outside [0, {n})")
        return t.to(torch.int32).contiguous()

    def _start(self, B, N, start_index, seed):
        import torch

        if start_index is not None and seed is not None:
            raise ValueError("give start_index or seed, not both")
        if seed is not None:
            g = torch.Generator().manual_seed(int(seed))
            return torch.randint(0, N, (B,), generator=g)
        if start_index is None:
            return torch.zeros(B, dtype=torch.long)
        s = torch.as_tensor(start_index).reshape(-1).cpu()
        return s.expand(B) if s.numel() == 1 else s

    def fps(self, points, num: Optional[int] = None, start_index=None, seed=None):
        """farthest-point sampling: (B, N, C) -> indices (B, num) int64, [:, 0] the start index (num: num_group by default)"""
        import torch

        from ..hip_backend import _stream_ptr

        p = self._points(points)
        B, N, C = p.shape
        G = self.cfg["num_group"] if num is None else int(num)
        if not 1 <= G <= N:
            raise ValueError(f"fps: cannot sample {G} of {N} points")
        start = self._indices("start_index", self._start(B, N, start_index, seed), (B,), N)
        out = torch.empty((B, G), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _check(self._lib.tamf_pointenc_fps(p.data_ptr(), start.data_ptr(), B, N, C, G, out.data_ptr(), _stream_ptr(self.device)))
        return out.long()

    def group(self, points, centre_idx, group_size: Optional[int] = None):
        """the group_size nearest points of every centre: -> (B, G, group_size) int64 in ascending (distance, index) order"""
        import torch

        from ..hip_backend import _stream_ptr

        p = self._points(points)
        B, N, C = p.shape
        M = self.cfg["group_size"] if group_size is None else int(group_size)
        if not 1 <= M <= N:
            raise ValueError(f"group: cannot take {M} of {N} points")
        ci = torch.as_tensor(centre_idx)
        if ci.dim() != 2 or ci.shape[0] != B or ci.shape[1] < 1:
            raise ValueError(f"centre_idx: expected ({B}, G), got {tuple(ci.shape)}")
        ci = self._indices("centre_idx", ci, ci.shape, N)
        G = int(ci.shape[1])
        out = torch.empty((B, G, M), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _check(self._lib.tamf_pointenc_group(p.data_ptr(), ci.data_ptr(), B, N, C, G, M, out.data_ptr(), _stream_ptr(self.device)))
        return out.long()

    def encode_groups(self, points, centre_idx, nbr_idx):
        """the encoder on given groups: points (B, N, point_dims), centre_idx (B, num_group), nbr_idx (B, num_group, group_size)
        -> (B, 2 * trans_dim) float32 on the device"""
        import torch

        from ..hip_backend import _stream_ptr

        if not self._loaded:
            raise PointEncoderError("no weights loaded")
        p = self._points(points, self.cfg["point_dims"])
        B, N, _ = p.shape
        G, M = self.cfg["num_group"], self.cfg["group_size"]
        ci = self._indices("centre_idx", centre_idx, (B, G), N)
        ni = self._indices("nbr_idx", nbr_idx, (B, G, M), N)
        out = torch.empty((B, self.out_dim), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            nb = min(B, MAX_CLOUDS_PER_CALL)
            nbytes = int(self._lib.tamf_pointenc_workspace_bytes(self._model, nb))
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
            for b0 in range(0, B, nb):
                n = min(nb, B - b0)
                _check(self._lib.tamf_pointenc_encode(self._model, p[b0:].data_ptr(), ci[b0:].data_ptr(), ni[b0:].data_ptr(), n, N,
                                                                out[b0:].data_ptr(), ws.data_ptr(), nbytes, _stream_ptr(self.device)))
        return out

    def encode(self, points, start_index=None, seed=None):
        """(B, N, point_dims) or (N, point_dims) -> (B, 2 * trans_dim): fps from `start_index` (or a draw from `seed`; default index
        0), grouping, encoder"""
        p = self._points(points, self.cfg["point_dims"])
        centre = self.fps(p, start_index=start_index, seed=seed)
        return self.encode_groups(p, centre, self.group(p, centre))

    __call__ = encode


__all__ = ["HipPointEncoder", "PointEncoderError", "DEFAULT_CFG", "PREFIX", "make_cfg", "expected_shapes", "map_checkpoint", "fold_bn", "fps_indices"]
