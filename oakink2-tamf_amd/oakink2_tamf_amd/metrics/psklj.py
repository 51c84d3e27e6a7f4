"""PSKL-J: power-spectrum KL divergence of joint accelerations (reference script/compute_score/compute_score_psklj.py:270-317).

power_spectrum_sum  :270-271 tail hold, :280-285 np.diff(n=2) -> fft -> |.|^2, :305 sum over clips - on the GPU through
                    tamf_power_spectrum_sum (csrc/tamf_spectrum.h): float32 second differences in numpy's order, a float64 direct DFT, the
                    clips added in order without atomics, so the bits do not depend on how N is chunked
pskl_terms          :305-316 on the host in float64: + 1e-8, normalise along the frequency axis, the two KL sums
No CPU fallback for the spectra, as in geometry.py."""
from __future__ import annotations

from ctypes import c_int32, c_void_p
from typing import Dict, Optional, Sequence

import numpy as np

EPS = 1e-8  # :305-306
DEFAULT_CHUNK = 1024  # clips per library call (the call itself takes any N; a chunk bounds the float32 staging copy on the device)


def _lib():
    from ..hip_backend import lib

    L = lib()
    L.tamf_power_spectrum_sum.argtypes = [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]
    return L


def power_spectrum_sum(joints, lens: Optional[Sequence[int]] = None, chunk: int = DEFAULT_CHUNK, return_clip: bool = False):
    """joints (N, T, J, 3) or (N, T, F) - a tensor, or a sequence of N clips (T, J, 3) of equal T (unequal T: ValueError, as the
    reference's np.stack) - and per-clip valid lengths in [1, T] (None: all T) -> float64 (T - 2, F) on the joints' device: the sum
    over clips of |DFT(second difference)|^2, frames from `len` on held at frame len - 1.  With return_clip also the per-clip spectra
    (N, T - 2, F) float64 (the reference's `dataset_psd`)."""
    import torch

    from ..hip_backend import _check, _dev_f32, _stream_ptr, require_gpu

    if not isinstance(joints, torch.Tensor):
        clips = [torch.as_tensor(np.asarray(c) if not isinstance(c, torch.Tensor) else c) for c in joints]
        if len({tuple(c.shape) for c in clips}) > 1:
            raise ValueError(f"power_spectrum_sum: clips of unequal shape {sorted({tuple(c.shape) for c in clips})} cannot be stacked")
        if not clips:
            raise ValueError("power_spectrum_sum: no clips")
        joints = torch.stack(clips, dim=0)
    if joints.dim() not in (3, 4):
        raise ValueError(f"power_spectrum_sum: joints must be (N, T, J, 3) or (N, T, F), got {tuple(joints.shape)}")
    dev = require_gpu(joints.device if joints.device.type == "cuda" else None)
    N, T = int(joints.shape[0]), int(joints.shape[1])
    x = joints.reshape(N, T, -1)
    F = int(x.shape[2])
    len_np = None
    if lens is not None:
        len_np = np.ascontiguousarray(np.asarray(lens, dtype=np.int64).reshape(-1))
        if len_np.shape[0] != N:
            raise ValueError(f"power_spectrum_sum: {len_np.shape[0]} lengths for {N} clips")
        if N and (len_np.min() < 1 or len_np.max() > T):
            raise ValueError(f"power_spectrum_sum: clip lengths must lie in [1, {T}]")
        len_np = len_np.astype(np.int32)
    chunk = max(1, int(chunk))
    L = _lib()
    psd_sum = torch.zeros((max(T - 2, 0), F), device=dev, dtype=torch.float64)
    psd_clip = torch.empty((N, max(T - 2, 0), F), device=dev, dtype=torch.float64) if return_clip else None
    with torch.cuda.device(dev):
        for s in range(0, max(N, 1), chunk):
            n = min(chunk, N - s)
            xs = _dev_f32(x[s: s + n], dev)
            lp = len_np[s: s + n].ctypes.data_as(c_void_p) if len_np is not None else c_void_p(0)
            pc = c_void_p(psd_clip[s: s + n].data_ptr()) if (psd_clip is not None and n > 0) else c_void_p(0)
            _check(L.tamf_power_spectrum_sum(c_void_p(xs.data_ptr()), lp, n, T, F, int(s > 0), c_void_p(psd_sum.data_ptr()), pc,
                                             c_void_p(_stream_ptr(dev))), None, L)
    return (psd_sum, psd_clip) if return_clip else psd_sum


def pskl_terms(psd_sum_dataset, psd_sum_model) -> Dict[str, float]:
    """The two scores from the summed spectra of the two sets, float64 on the host, the reference's operations in its order (:305-316).
    The arrays keep the shape the reference has at that point, (T - 2, J, 3) - frequency first; `num_feat` is the reference's
    `shape[1]`, i.e. the number of JOINTS for (L, J, 3) input (and the number of columns for a flat (L, F) array)."""
    d = np.asarray(psd_sum_dataset.detach().cpu().numpy() if hasattr(psd_sum_dataset, "detach") else psd_sum_dataset, dtype=np.float64)
    m = np.asarray(psd_sum_model.detach().cpu().numpy() if hasattr(psd_sum_model, "detach") else psd_sum_model, dtype=np.float64)
    if d.shape != m.shape or d.ndim < 2:
        raise ValueError(f"pskl_terms: summed spectra of shapes {d.shape} and {m.shape}")
    d = d + EPS
    m = m + EPS
    d = d / np.sum(d, axis=0, keepdims=True)
    m = m / np.sum(m, axis=0, keepdims=True)
    num_feat = d.shape[1]
    pskl_1 = 1 / num_feat * np.sum(d * np.log(d / m))
    pskl_2 = 1 / num_feat * np.sum(m * np.log(m / d))
    return {"pskl_gt_model": float(pskl_1), "pskl_model_gt": float(pskl_2), "n_freq": int(d.shape[0]), "n_feat": int(num_feat)}
