"""Kernel Inception distance (Binkowski et al. 2018) from extractor features, as the reference's ``kid_features_to_metric``
(metrics/metric_kid.py) computes it: the unbiased MMD^2 under the polynomial kernel ``(gamma <a, b> + coef0)^degree`` of ``subsets``
random subsets of ``subset_size`` features from either set; mean and ``np.std`` over the subsets.

``kid_indices`` draws the subsets as the reference does (one ``RandomState``, per subset ``choice`` without replacement from set 1,
then from set 2), so they are the reference's own.  ``kid_sums`` is one ``adm_kid_sums`` launch (adm_amd/csrc/kid.hip) for all
subsets: the features stay on the device, the rows are gathered through the index tables inside the kernel, and per subset the three
kernel sums come back in float64 -- the same bits every run.  ``mmd_from_sums`` is the host half.

Stated deviation: the reference forms ``K``, ``K ** degree`` and the sums in NumPy float32.  Here the dot product is float32 (the
exact f32 MFMA, an fmaf chain) and everything after it is float64.  Only the ``'unbiased'`` estimator exists, the one the reference
reaches.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .. import hip
from ..hip import call, ptr

KEY_KID_MEAN = "kernel_inception_distance_mean"
KEY_KID_STD = "kernel_inception_distance_std"
SUBSETS, SUBSET_SIZE, DEGREE, GAMMA, COEF0, RNG_SEED = 100, 1000, 3, None, 1, 2020          # metrics/defaults.py of the reference


def check_subset_size(n1: int, n2: int, subset_size: int) -> None:
    if not (n1 >= subset_size and n2 >= subset_size):
        raise ValueError(f"KID subset size {subset_size} cannot be smaller than the number of samples (input_1: {n1}, "
                         f"input_2: {n2}). Consider using \"kid_subset_size\" kwarg or \"--kid-subset-size\" command line key to "
                         "proceed.")


def kid_indices(n1: int, n2: int, subsets: int = SUBSETS, subset_size: int = SUBSET_SIZE,
                rng_seed: int = RNG_SEED) -> Tuple[np.ndarray, np.ndarray]:
    """-> (idx1, idx2), int32 [subsets, subset_size]: the rows of set 1 / set 2 in each subset, in the reference's draw order."""
    check_subset_size(n1, n2, subset_size)
    if subsets < 1 or subset_size < 2:
        raise ValueError(f"KID needs at least 1 subset of at least 2 samples, got {subsets} of {subset_size}")
    rng = np.random.RandomState(rng_seed)
    idx1 = np.empty((subsets, subset_size), np.int32)
    idx2 = np.empty((subsets, subset_size), np.int32)
    for s in range(subsets):
        idx1[s] = rng.choice(n1, subset_size, replace=False)
        idx2[s] = rng.choice(n2, subset_size, replace=False)
    return idx1, idx2


def check_indices(idx, n: int, what: str = "idx") -> np.ndarray:
    """An integer [S, m] table with every entry in [0, n), as contiguous int32; raises with the offending value otherwise."""
    a = np.asarray(idx.cpu() if torch.is_tensor(idx) else idx)
    if a.ndim != 2 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what} must be an integer [subsets, subset_size] table, got {a.dtype} {a.shape}")
    bad = (a < 0) | (a >= n)
    if bad.any():
        s, j = np.argwhere(bad)[0]
        raise IndexError(f"{what}[{s}, {j}] = {int(a[s, j])} is outside the {n} feature rows")
    return np.ascontiguousarray(a, dtype=np.int32)


@torch.no_grad()
def kid_sums(f1: torch.Tensor, f2: torch.Tensor, idx1, idx2, degree: int = DEGREE, gamma: Optional[float] = GAMMA,
             coef0: float = COEF0) -> torch.Tensor:
    """f1 [n1, D], f2 [n2, D] float32 on the GPU, idx1 / idx2 integer [S, m] -> float64 [S, 3] on the GPU: per subset
    sum_{i != j} k(X_i, X_j), sum_{i != j} k(Y_i, Y_j), sum_{i, j} k(X_i, Y_j) for X = f1[idx1[s]], Y = f2[idx2[s]]."""
    if not (torch.is_tensor(f1) and torch.is_tensor(f2)):
        raise TypeError("the features must be torch tensors on the GPU")
    hip.require_cuda(f1, "the first feature matrix")
    hip.require_cuda(f2, "the second feature matrix")
    if f1.dim() != 2 or f2.dim() != 2 or f1.shape[1] != f2.shape[1]:
        raise ValueError(f"the features must be [n1, D] and [n2, D], got {tuple(f1.shape)} and {tuple(f2.shape)}")
    if f1.dtype != torch.float32 or f2.dtype != torch.float32:
        raise ValueError(f"the features must be float32, got {f1.dtype} and {f2.dtype}")
    n1, n2, D = int(f1.shape[0]), int(f2.shape[0]), int(f1.shape[1])
    t1, t2 = check_indices(idx1, n1, "idx1"), check_indices(idx2, n2, "idx2")         # raises before any launch
    if t1.shape != t2.shape:
        raise ValueError(f"idx1 and idx2 must have one shape, got {t1.shape} and {t2.shape}")
    S, m = t1.shape
    if D % 4 != 0:
        raise ValueError(f"the feature width must be a multiple of 4, got {D}")
    if S < 1 or m < 2 or m > min(n1, n2):
        raise ValueError(f"need at least 1 subset and 2 <= subset size <= min(n1, n2) = {min(n1, n2)}, got {S} subsets of {m}")
    degree = int(degree)
    if not 1 <= degree <= 8:
        raise ValueError(f"the kernel's degree must be an integer from 1 to 8, got {degree}")
    gamma = 1.0 / D if gamma is None else float(gamma)
    f1, f2 = f1.contiguous(), f2.contiguous()
    dev = f1.device
    d1, d2 = torch.from_numpy(t1).to(dev), torch.from_numpy(t2).to(dev)
    blocks = int(hip.lib().adm_kid_sums_blocks(m))
    sums = torch.empty(S, 3, device=dev, dtype=torch.float64)
    partial = torch.empty(S, blocks, device=dev, dtype=torch.float64)
    call("adm_kid_sums", ptr(f1), n1, ptr(f2), n2, D, ptr(d1), ptr(d2), S, m, degree, gamma, float(coef0), ptr(sums), ptr(partial))
    return sums


def mmd_from_sums(sums, m: int) -> np.ndarray:
    """float64 [S, 3] sums -> float64 [S]: (s_xx + s_yy) / (m (m - 1)) - 2 s_xy / m^2, the reference's 'unbiased' mmd2."""
    s = np.asarray(sums.cpu() if torch.is_tensor(sums) else sums, dtype=np.float64).reshape(-1, 3)
    m = int(m)
    return (s[:, 0] + s[:, 1]) / (m * (m - 1)) - 2 * s[:, 2] / (m * m)


def kid_from_mmds(mmds) -> Dict[str, float]:
    mmds = np.asarray(mmds, dtype=np.float64)
    return {KEY_KID_MEAN: float(np.mean(mmds)), KEY_KID_STD: float(np.std(mmds))}


def kid_from_features(f1: torch.Tensor, f2: torch.Tensor, subsets: int = SUBSETS, subset_size: int = SUBSET_SIZE,
                      degree: int = DEGREE, gamma: Optional[float] = GAMMA, coef0: float = COEF0,
                      rng_seed: int = RNG_SEED) -> Dict[str, float]:
    """Mean and std of the per-subset MMD^2 of two feature sets on the GPU; ``gamma=None`` means 1 / D."""
    if f1.dim() != 2 or f2.dim() != 2 or f1.shape[1] != f2.shape[1]:
        raise ValueError(f"the features must be [n1, D] and [n2, D], got {tuple(f1.shape)} and {tuple(f2.shape)}")
    idx1, idx2 = kid_indices(int(f1.shape[0]), int(f2.shape[0]), subsets, subset_size, rng_seed)
    sums = kid_sums(f1, f2, idx1, idx2, degree, gamma, coef0)
    return kid_from_mmds(mmd_from_sums(sums, subset_size))
