"""Fréchet distance between two sets of encoder features (the FID score of the reference's
script/compute_score/compute_score_fid.py:142-206), float64 on the host.

Each set is summarised by a Gaussian - its sample mean and its unbiased sample covariance - and the score is the squared 2-Wasserstein
distance between the two Gaussians:

    FID = |mu_1 - mu_2|^2 + tr(S_1) + tr(S_2) - 2 tr((S_1 S_2)^(1/2))

The matrix square root is scipy.linalg.sqrtm.  When the product S_1 S_2 is close to singular that square root can come out non-finite;
the computation is then repeated with eps added to both diagonals.  A small imaginary part left by sqrtm (numerical noise) is dropped,
a large one on the diagonal (|Im| > 1e-3) is an error.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np


def calculate_activation_statistics(activations) -> Tuple[np.ndarray, np.ndarray]:
    """(N, d) features -> (mean (d,), covariance (d, d)), both float64; the covariance has rows = observations and the N - 1
    normalisation of numpy.cov(rowvar=False)."""
    a = np.asarray(activations, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError(f"expected an (N, d) array of features, got shape {a.shape}")
    return a.mean(axis=0), np.cov(a, rowvar=False)


def frechet_distance_terms(mu1, sigma1, mu2, sigma2, eps: float = 1e-6) -> Dict[str, float]:
    """The score and its four terms: {"fid", "mean_sq_diff", "trace_sigma1", "trace_sigma2", "trace_covmean"}."""
    from scipy import linalg

    mu1, mu2 = np.atleast_1d(np.asarray(mu1, dtype=np.float64)), np.atleast_1d(np.asarray(mu2, dtype=np.float64))
    s1, s2 = np.atleast_2d(np.asarray(sigma1, dtype=np.float64)), np.atleast_2d(np.asarray(sigma2, dtype=np.float64))
    if mu1.shape != mu2.shape:
        raise ValueError(f"mean vectors differ in length: {mu1.shape} vs {mu2.shape}")
    if s1.shape != s2.shape:
        raise ValueError(f"covariances differ in shape: {s1.shape} vs {s2.shape}")
    delta = mu1 - mu2
    root, _ = linalg.sqrtm(s1.dot(s2), disp=False)
    if not np.isfinite(root).all():
        print(f"fid: the covariance product is close to singular; retrying with {eps} added to both diagonals")
        shift = np.eye(s1.shape[0]) * eps
        root = linalg.sqrtm((s1 + shift).dot(s2 + shift))
    if np.iscomplexobj(root):
        if not np.allclose(np.diagonal(root).imag, 0, atol=1e-3):
            raise ValueError(f"fid: the matrix square root has an imaginary part of up to {np.max(np.abs(root.imag))}")
        root = root.real
    terms = {"mean_sq_diff": float(delta.dot(delta)), "trace_sigma1": float(np.trace(s1)), "trace_sigma2": float(np.trace(s2)),
             "trace_covmean": float(np.trace(root))}
    terms["fid"] = float(delta.dot(delta) + np.trace(s1) + np.trace(s2) - 2 * np.trace(root))
    return terms


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps: float = 1e-6) -> float:
    """FID of two Gaussians given by (mean, covariance); see the module docstring."""
    return frechet_distance_terms(mu1, sigma1, mu2, sigma2, eps)["fid"]


def calculate_fid(statistics_1, statistics_2) -> float:
    """FID of two (mean, covariance) pairs as returned by calculate_activation_statistics."""
    return calculate_frechet_distance(statistics_1[0], statistics_1[1], statistics_2[0], statistics_2[1])
