"""The depth-estimation score: abs-rel / sq-rel / RMSE / RMSE-log / SILog / log10 / delta < 1.25^k, as the field reports them (Eigen et
al. 2014; the evaluation of BTS, AdaBins and their successors).

``depth_sums`` is one ``adm_depth_metrics`` launch (adm_amd/csrc/depth_data.hip): per image the float64 sums over the valid pixels,
added in a fixed order -- the same bits every run.  ``metrics_from_sums`` is the host half: every metric is computed per image and
then averaged over the images; an image without a valid pixel is skipped and counted.

Depths are FRACTIONS of 10 m, as the depth recipe's model predicts them and its 16-bit files store them (fraction 1.0 = 10000 raw
units = 10 m); the metrics are in metres.  With p the prediction clamped to [min_depth, max_depth], g the ground truth, over the n
pixels with min_depth < g < max_depth (defaults 1e-3 and 10, NYUv2's):
  abs_rel = mean |p - g| / g            sq_rel = mean (p - g)^2 / g          rmse = sqrt(mean (p - g)^2)
  rmse_log = sqrt(mean (ln p - ln g)^2)   silog = 100 sqrt(mean e^2 - (mean e)^2), e = ln p - ln g
  log10 = mean |log10 p - log10 g|      d_k = share of pixels with max(p/g, g/p) < 1.25^k
No further crop is taken: the box the dataset applies is the Eigen evaluation crop.
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch

from .. import hip
from ..hip import call, ptr

KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "silog", "log10", "d1", "d2", "d3")
N_SUMS = 10          # ADM_DEPTH_SUMS of include/adm_hip.h
MIN_DEPTH, MAX_DEPTH = 1e-3, 10.0


@torch.no_grad()
def depth_sums(pred: torch.Tensor, gt: torch.Tensor, min_depth: float = MIN_DEPTH, max_depth: float = MAX_DEPTH) -> torch.Tensor:
    """pred / gt float32 [B,1,H,W] depth fractions on the GPU -> float64 [B, 10] on the GPU: {n, S|p-g|/g, S(p-g)^2/g, S(p-g)^2,
    S(ln p - ln g)^2, S(ln p - ln g), S|log10 p - log10 g|, #[r < 1.25], #[r < 1.25^2], #[r < 1.25^3]}."""
    hip.require_cuda(pred, "the prediction")
    hip.require_cuda(gt, "the ground truth")
    if pred.shape != gt.shape or pred.dim() != 4 or pred.shape[1] != 1:
        raise ValueError(f"pred and gt must both be [B,1,H,W], got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise ValueError(f"pred and gt must be float32, got {pred.dtype} and {gt.dtype}")
    pred, gt = pred.contiguous(), gt.contiguous()
    B, hw = int(pred.shape[0]), int(pred.shape[2] * pred.shape[3])
    blocks = int(hip.lib().adm_depth_metrics_blocks(hw))
    sums = torch.empty(B, N_SUMS, device=pred.device, dtype=torch.float64)
    partial = torch.empty(B, blocks, N_SUMS, device=pred.device, dtype=torch.float64)
    ticket = torch.zeros(B, device=pred.device, dtype=torch.int32)
    call("adm_depth_metrics", ptr(pred), ptr(gt), ptr(sums), ptr(partial), ptr(ticket), B, hw, float(min_depth), float(max_depth))
    return sums


def per_image(sums) -> np.ndarray:
    """float64 [N, 10] sums -> float64 [N, 9] metrics in the order of ``KEYS``; a row without a valid pixel is NaN."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, N_SUMS)
    out = np.full((s.shape[0], len(KEYS)), np.nan)
    ok = s[:, 0] > 0
    n = s[ok, 0]
    mean_e, mean_e2 = s[ok, 5] / n, s[ok, 4] / n
    out[ok] = np.stack([s[ok, 1] / n, s[ok, 2] / n, np.sqrt(s[ok, 3] / n), np.sqrt(mean_e2),
                        100.0 * np.sqrt(np.maximum(mean_e2 - mean_e ** 2, 0.0)), s[ok, 6] / n, s[ok, 7] / n, s[ok, 8] / n,
                        s[ok, 9] / n], axis=1)
    return out


def metrics_from_sums(sums) -> Dict[str, float]:
    """The nine metrics averaged over the images that have a valid pixel, plus ``images`` (how many those are) and ``skipped`` (how many
    have none).  With no scored image the metrics are NaN."""
    m = per_image(sums)
    ok = ~np.isnan(m[:, 0])
    res = {k: (float(m[ok, i].mean()) if ok.any() else math.nan) for i, k in enumerate(KEYS)}
    res["images"], res["skipped"] = int(ok.sum()), int((~ok).sum())
    return res


class DepthScore:
    """Accumulates ``depth_sums`` of batches on the device; ``result()`` makes the one host copy."""

    def __init__(self, min_depth: float = MIN_DEPTH, max_depth: float = MAX_DEPTH):
        self.min_depth, self.max_depth, self.sums = float(min_depth), float(max_depth), []

    def add(self, pred: torch.Tensor, gt: torch.Tensor):
        self.sums.append(depth_sums(pred, gt, self.min_depth, self.max_depth))

    def result(self) -> Dict[str, float]:
        if not self.sums:
            return metrics_from_sums(np.zeros((0, N_SUMS)))
        return metrics_from_sums(torch.cat(self.sums).cpu().numpy())
