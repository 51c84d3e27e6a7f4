"""float64 numpy restatements of the two scores the launchers compute_score_cr / compute_score_psklj print (not tests).

PSKL-J (reference script/compute_score/compute_score_psklj.py:270-317): tail hold, np.diff(n=2) on the float32 joints, np.fft.fft of
the float64 cast, |.|^2, sum over clips, + 1e-8, normalise along frequency, the two KL sums.  The reference transforms the float32
accelerations as they are (its numpy computes that FFT in float32); here the transform is float64, which is what the kernel is held to.
CR (compute_score_cr.py:268-285) on oracle.geometry_oracle.contact_min_dist in float64."""
import numpy as np


def hold_tail(joints, lens=None):
    """(N, T, ...) float32 -> copy with frames t >= len[n] set to frame len[n] - 1 (:270-271)"""
    x = np.array(joints, dtype=np.float32, copy=True)
    if lens is not None:
        for n, l in enumerate(lens):
            x[n, int(l):] = x[n, int(l) - 1]
    return x


def accelerations(joints, lens=None):
    """float32 second differences along time, numpy's order (np.diff(n=2) = diff of diff)"""
    return np.diff(hold_tail(joints, lens), n=2, axis=1)


def clip_spectra(joints, lens=None):
    """(N, T, ...) -> float64 (N, T - 2, ...): |fft(acc)|^2 per clip (:280-285 with a float64 transform)"""
    acc = accelerations(joints, lens).astype(np.float64)
    f = np.fft.fft(acc, axis=1)
    return f.real ** 2 + f.imag ** 2


def spectrum_sum(joints, lens=None):
    return clip_spectra(joints, lens).sum(axis=0)


def direct_dft_spectra(joints, lens=None):
    """the same by a direct float64 DFT with exact-index twiddles: cos / sin of 2 pi ((k n) mod L) / L - the arithmetic of the kernel,
    used to MEASURE how far a correct direct transform sits from np.fft.fft on given inputs"""
    acc = accelerations(joints, lens).astype(np.float64)
    L = acc.shape[1]
    j = (np.arange(L)[:, None] * np.arange(L)[None, :]) % L
    ang = 2.0 * np.pi * j / L
    c, s = np.cos(ang), np.sin(ang)
    flat = acc.reshape(acc.shape[0], L, -1)
    re = np.einsum("kn,bnf->bkf", c, flat)
    im = np.einsum("kn,bnf->bkf", s, flat)
    return (re ** 2 + im ** 2).reshape(acc.shape)


def rel_to_feature_max(a, b):
    """max |a - b| relative to each feature's largest bin of b; a, b (..., L, F...) with the frequency axis at -2 for flat (L, F) or
    given explicitly as axis 0 of a summed spectrum.  Features whose spectrum is identically zero compare absolutely (must be equal)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    L = a.shape[0]
    a2, b2 = a.reshape(L, -1), b.reshape(L, -1)
    scale = np.abs(b2).max(axis=0)
    d = np.abs(a2 - b2).max(axis=0)
    if np.any((scale == 0) & (d != 0)):
        return np.inf
    return float(np.max(np.where(scale > 0, d / np.where(scale > 0, scale, 1.0), 0.0))) if d.size else 0.0


def pskl(psd_sum_dataset, psd_sum_model):
    """(:305-316) on summed spectra shaped as the reference has them, (L, J, 3): num_feat is shape[1]"""
    d = np.asarray(psd_sum_dataset, np.float64) + 1e-8
    m = np.asarray(psd_sum_model, np.float64) + 1e-8
    d = d / np.sum(d, axis=0, keepdims=True)
    m = m / np.sum(m, axis=0, keepdims=True)
    nf = d.shape[1]
    return float(1 / nf * np.sum(d * np.log(d / m))), float(1 / nf * np.sum(m * np.log(m / d)))


def contact_distances(items, verts):
    """float64 per-frame contact distances of the first `len` frames of every clip, concatenated in order (compute_score_cr.py:268-277)"""
    import torch

    from oracle import geometry_oracle as G

    out = []
    for it, v in zip(items, verts):
        n = int(it["len"])
        hv = torch.from_numpy(np.asarray(v, np.float64)[None, :n])
        traj = torch.from_numpy(np.asarray(it["obj_traj"], np.float64)[None, :, :n])
        pts = torch.from_numpy(np.asarray(it["obj_pointcloud"], np.float64)[None])
        out.append(G.contact_min_dist(hv, traj, pts).numpy()[0])
    return np.concatenate(out, axis=0)
