"""Frechet Inception distance and Inception score from extractor features.

``FeatureStats`` streams feature batches into ``adm_feat_stats_accum`` (csrc/inception.hip): float64 sums of ``x - c`` and of their
outer products on the device, ``c`` being the column mean of the first batch, so a large common offset cannot cancel digits.  The
host then forms ``mu = c + sum / N`` and ``sigma = (outer - sum sum^T / N) / (N - 1)`` in float64.

``fid_from_stats`` and ``inception_score`` follow the reference's ``fid_statistics_to_metric`` (metrics/metric_fid.py) and
``isc_features_to_metric`` (metrics/metric_isc.py).  Stated deviation: the reference's ``mu`` is a float32 ``np.mean``; ours is
float64.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from .. import hip

KEY_FID = "frechet_inception_distance"
KEY_ISC_MEAN = "inception_score_mean"
KEY_ISC_STD = "inception_score_std"

Stats = namedtuple("Stats", ("mu", "sigma", "n"))


class FeatureStats:
    """Streaming mean and covariance of [n, D] float32 feature batches on the GPU."""

    def __init__(self, D: int, device="cuda"):
        self.D, self.n = int(D), 0
        dev = torch.device(device)
        self.shift = torch.zeros(self.D, dtype=torch.float64, device=dev)
        self.sum = torch.zeros(self.D, dtype=torch.float64, device=dev)
        self.outer = torch.zeros(self.D, self.D, dtype=torch.float64, device=dev)

    def update(self, feats: torch.Tensor) -> None:
        hip.require_cuda(feats, "feature batch")
        if feats.dim() != 2 or feats.shape[1] != self.D or feats.dtype != torch.float32:
            raise ValueError(f"expected float32 [n, {self.D}] features, got {feats.dtype} {tuple(feats.shape)}")
        if feats.shape[0] == 0:
            return
        feats = feats.contiguous()
        hip.call("adm_feat_stats_accum", hip.ptr(feats), feats.shape[0], self.D, hip.ptr(self.shift), hip.ptr(self.sum),
                 hip.ptr(self.outer), 1 if self.n == 0 else 0)
        self.n += feats.shape[0]

    def finalize(self) -> Stats:
        if self.n < 2:
            raise ValueError(f"a covariance needs at least 2 samples, got {self.n}")
        c, s, o = (t.cpu().numpy() for t in (self.shift, self.sum, self.outer))
        mu = c + s / self.n
        sigma = (o - np.outer(s, s) / self.n) / (self.n - 1)
        return Stats(mu, sigma, self.n)

    def save(self, path: str) -> Stats:
        st = self.finalize()
        save_stats(path, st)
        return st

    @staticmethod
    def load(path: str) -> Stats:
        return load_stats(path)


def save_stats(path: str, st: Stats) -> None:
    with open(path, "wb") as f:            # (an open file: np.savez would append ".npz" to a bare name)
        np.savez(f, mu=np.asarray(st.mu, np.float64), sigma=np.asarray(st.sigma, np.float64), n=np.int64(st.n))


def load_stats(path: str) -> Stats:
    with np.load(path) as z:
        return Stats(z["mu"].astype(np.float64), z["sigma"].astype(np.float64), int(z["n"]) if "n" in z.files else -1)


def _mu_sigma(s):
    if isinstance(s, dict):
        return np.asarray(s["mu"], np.float64), np.asarray(s["sigma"], np.float64)
    if isinstance(s, FeatureStats):
        s = s.finalize()
    return np.asarray(s.mu, np.float64), np.asarray(s.sigma, np.float64)


def fid_from_stats(s1, s2, eps: float = 1e-6) -> float:
    """|mu1 - mu2|^2 + tr(S1) + tr(S2) - 2 tr(sqrtm(S1 S2)) with scipy's sqrtm; when the root is not finite, ``eps`` is added to both
    diagonals first; a root whose diagonal has an imaginary part beyond 1e-3 is an error, a smaller one is dropped."""
    import scipy.linalg
    mu1, sg1 = _mu_sigma(s1)
    mu2, sg2 = _mu_sigma(s2)
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sg1, sg2 = np.atleast_2d(sg1), np.atleast_2d(sg2)
    if mu1.shape != mu2.shape or sg1.shape != sg2.shape:
        raise ValueError(f"statistics of different sizes: {mu1.shape} / {mu2.shape}, {sg1.shape} / {sg2.shape}")
    d = mu1 - mu2
    root = scipy.linalg.sqrtm(sg1.dot(sg2), disp=False)[0]
    if not np.isfinite(root).all():
        off = np.eye(sg1.shape[0]) * eps
        root = scipy.linalg.sqrtm((sg1 + off).dot(sg2 + off), disp=False)[0]
    if np.iscomplexobj(root):
        if not np.allclose(np.diagonal(root).imag, 0, atol=1e-3):
            raise ValueError(f"sqrtm has an imaginary component of {np.max(np.abs(root.imag))}")
        root = root.real
    return float(d.dot(d) + np.trace(sg1) + np.trace(sg2) - 2 * np.trace(root))


def inception_score(logits, splits: int = 10, shuffle: bool = True, rng_seed: int = 2020) -> dict:
    """exp(mean_x KL(p(y|x) || p(y))) over ``splits`` consecutive chunks of the (shuffled) rows, in float64: mean and std."""
    x = logits.detach().cpu() if torch.is_tensor(logits) else torch.as_tensor(np.asarray(logits))
    if x.dim() != 2:
        raise ValueError("logits must be [N, classes]")
    N = x.shape[0]
    if shuffle:
        x = x[torch.from_numpy(np.random.RandomState(rng_seed).permutation(N))]
    x = x.double()
    p, logp = x.softmax(dim=1), x.log_softmax(dim=1)
    scores = []
    for i in range(splits):
        lo, hi = i * N // splits, (i + 1) * N // splits
        q = p[lo:hi].mean(dim=0, keepdim=True)
        scores.append((p[lo:hi] * (logp[lo:hi] - q.log())).sum(dim=1).mean().exp().item())
    return {KEY_ISC_MEAN: float(np.mean(scores)), KEY_ISC_STD: float(np.std(scores))}
