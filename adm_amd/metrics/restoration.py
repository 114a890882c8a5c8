"""The restoration score: PSNR and SSIM on RGB and on the Y channel, with a border shave -- the columns of every DIV2K x4
super-resolution table (Y, ``crop_border`` = scale) and every CelebA-HQ in-painting table (RGB, no shave).  The definitions are this
project's own; they follow the float path of the field's common evaluation code (BasicSR's ``calculate_psnr`` / ``calculate_ssim``).

Inputs.  Prediction p and target g are [B,C,H,W], C = 1 or 3, each uint8 (used as it is) or float32 in [0, 1], quantised in the kernel
as rintf(fminf(fmaxf(v, 0), 1) * 255), ties to even, NaN -> 0: adm_saliency_tables' rule, the bytes ``save_prediction`` writes.
Shave.  ``crop_border`` = s >= 0 pixels are dropped from every side: the scored area is H' x W' = (H - 2s) x (W - 2s); addressing only.
Planes.  C = 3: R, G, B and Y = 16 + N / 255000 with the integer N = 65481 R + 128553 G + 24966 B -- BT.601 in Matlab's ``rgb2ycbcr``
coefficients, UNROUNDED.  C = 1: the one plane.
PSNR.  Per plane SSE = sum of d^2 over the area as an exact integer: d = p - g on a byte plane, N_p - N_g on Y (scaled by 255000^-2
here).  |N_p - N_g| < 2^26 and there are up to 2^24 pixels, so the sum can pass int64: the kernel returns two int64 words {lo, hi},
value = hi 2^32 + lo, reassembled here with Python integers.  psnr = 10 log10(255^2 / MSE), MSE over the three RGB planes together (the
one plane when C = 1); psnr_y the same from Y.  SSE = 0 gives ``inf``: kept, not clamped.
SSIM.  11 x 11 Gaussian window, sigma 1.5, normalised to sum 1, the outer product of the 1-D window; VALID region only, (H' - 10) x
(W' - 10) positions, no padding.  mu = w*x, sigma_x^2 = w*x^2 - mu_x^2, sigma_xy = w*xy - mu_x mu_y, C1 = 6.5025, C2 = 58.5225; per
position (2 mu_p mu_g + C1)(2 sigma_pg + C2) / ((mu_p^2 + mu_g^2 + C1)(sigma_p^2 + sigma_g^2 + C2)); a plane's value is the mean over
the positions; ssim the mean over R, G, B (the one plane when C = 1), ssim_y the Y plane's.
Every metric is computed per image and then averaged over the images.

``restoration_sums`` is one ``adm_restoration_sums`` launch (adm_amd/csrc/restoration_metrics.hip): the SSE words and the float64 SUM
of each plane's SSIM map, filtered in float64 and added in a fixed order -- the same bits every run.  ``per_image`` /
``metrics_from_sums`` are the host half, in float64.

Deviations from common evaluation code: Y is not rounded to a byte (Matlab's uint8 ``rgb2ycbcr`` rounds; tables made that way differ in
the second decimal); a float prediction is scored as the bytes its PNG holds, never as floats; an infinite PSNR of one image makes the
mean infinite.
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch

from .. import hip
from ..hip import call, ptr

KEYS = ("psnr", "ssim", "psnr_y", "ssim_y")
WINDOW = 11          # ADM_RESTORATION_WINDOW of include/adm_hip.h
MAX_PIXELS = 1 << 24          # ADM_RESTORATION_MAX_PIXELS
Y_SCALE = 255000


def planes_of(channels: int) -> int:
    return 4 if channels == 3 else 1


@torch.no_grad()
def restoration_sums(pred: torch.Tensor, target: torch.Tensor, crop_border: int = 0):
    """pred / target uint8 or float32 (in [0, 1]; quantised in the kernel) [B,C,H,W] on the GPU, C = 1 or 3 -> (sse int64 [B,P,2] --
    {lo, hi} words --, ssim float64 [B,P] -- the SUM over the valid positions --) on the GPU; P = 4 (R, G, B, Y) for C = 3, else 1."""
    hip.require_cuda(pred, "the prediction")
    hip.require_cuda(target, "the target")
    if pred.dim() != 4 or pred.shape != target.shape or pred.shape[1] not in (1, 3):
        raise ValueError(f"the prediction and the target must both be [B,C,H,W] with C = 1 or 3, got {tuple(pred.shape)} and {tuple(target.shape)}")
    for what, t in (("the prediction", pred), ("the target", target)):
        if t.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"{what} must be uint8 or float32, got {t.dtype}")
    s = int(crop_border)
    B, C, H, W = (int(v) for v in pred.shape)
    if s < 0:
        raise ValueError(f"crop_border must be >= 0, got {s}")
    if H - 2 * s < WINDOW or W - 2 * s < WINDOW:
        raise ValueError(f"a {H}x{W} image shaved by crop_border {s} leaves {H - 2 * s}x{W - 2 * s}: smaller than the "
                         f"{WINDOW}x{WINDOW} SSIM window")
    if not 1 <= B <= 65535 or H * W > MAX_PIXELS:
        raise ValueError(f"restoration_sums takes 1 .. 65535 images of up to 2^24 pixels, got {B} of {H}x{W}")
    pred, target = pred.contiguous(), target.contiguous()
    P = planes_of(C)
    blocks = int(hip.lib().adm_restoration_blocks(H - 2 * s, W - 2 * s))
    sse = torch.empty(B, P, 2, device=pred.device, dtype=torch.int64)
    ssim = torch.empty(B, P, device=pred.device, dtype=torch.float64)
    partial = torch.empty(B, blocks, P, 2, device=pred.device, dtype=torch.int64)
    ticket = torch.zeros(B, device=pred.device, dtype=torch.int32)
    call("adm_restoration_sums", ptr(pred), int(pred.dtype == torch.float32), ptr(target), int(target.dtype == torch.float32), ptr(sse),
         ptr(ssim), ptr(partial), ptr(ticket), B, C, H, W, s)
    return sse, ssim


def _psnr(sse: int, count: int, scale: int) -> float:
    """10 log10(255^2 / (sse / scale^2 / count)) of an integer sse over `count` values; inf for sse = 0."""
    if sse == 0:
        return math.inf
    # (the integers are divided as integers' ratio: one rounding, whatever their size)
    return 10.0 * math.log10((255 * 255 * scale * scale * count) / sse)


def per_image(sse, ssim, hw) -> Dict[str, np.ndarray]:
    """sse int64 [n,P,2], ssim float64 [n,P] (sums), hw = (H', W') of the shaved area or [n,2] -> {'psnr', 'ssim' (+ 'psnr_y', 'ssim_y' when
    P = 4): float64 [n]; 'ssim_planes': float64 [n,P]; 'sse_planes': object [n,P] of Python integers}."""
    words = np.asarray(sse, dtype=np.int64)
    P = int(words.shape[-2]) if words.ndim >= 2 else 1
    words = words.reshape(-1, P, 2)
    sums = np.asarray(ssim, dtype=np.float64).reshape(-1, P)
    n = words.shape[0]
    if P not in (1, 4) or sums.shape[0] != n:
        raise ValueError(f"sse {words.shape} and ssim {sums.shape} must be [n,P,2] and [n,P] with P = 1 or 4")
    sizes = np.broadcast_to(np.asarray(hw, dtype=np.int64).reshape(-1, 2), (n, 2))
    out = {k: np.zeros(n) for k in (KEYS if P == 4 else KEYS[:2])}
    out["ssim_planes"], out["sse_planes"] = np.zeros((n, P)), np.zeros((n, P), dtype=object)
    rgb = 3 if P == 4 else 1
    for i in range(n):
        H, W = int(sizes[i, 0]), int(sizes[i, 1])
        if H < WINDOW or W < WINDOW:
            raise ValueError(f"image {i}: a scored area of {H}x{W} is smaller than the {WINDOW}x{WINDOW} window")
        whole = [(int(words[i, p, 1]) << 32) + int(words[i, p, 0]) for p in range(P)]
        if any(not 0 <= int(words[i, p, 0]) < (1 << 32) or int(words[i, p, 1]) < 0 for p in range(P)):
            raise ValueError(f"image {i}: SSE words {words[i].tolist()} are not {{lo, hi}} with 0 <= lo < 2^32, hi >= 0")
        out["sse_planes"][i] = whole
        out["ssim_planes"][i] = sums[i] / ((H - WINDOW + 1) * (W - WINDOW + 1))
        out["psnr"][i] = _psnr(sum(whole[:rgb]), rgb * H * W, 1)
        out["ssim"][i] = out["ssim_planes"][i, :rgb].mean()
        if P == 4:
            out["psnr_y"][i] = _psnr(whole[3], H * W, Y_SCALE)
            out["ssim_y"][i] = out["ssim_planes"][i, 3]
    return out


def metrics_from_sums(sse, ssim, hw) -> Dict[str, float]:
    """psnr, ssim (and psnr_y, ssim_y for three channels) averaged over the images, plus ``images``; NaN without an image."""
    m = per_image(sse, ssim, hw)
    n = int(m["psnr"].shape[0])
    keys = [k for k in KEYS if k in m]
    if n == 0:
        return dict({k: math.nan for k in keys}, images=0)
    return dict({k: float(m[k].mean()) for k in keys}, images=n)


class RestorationScore:
    """Accumulates ``restoration_sums`` of batches on the device; ``result()`` makes the one host copy.  Every batch has the same
    channel count; sizes may differ."""

    def __init__(self, crop_border: int = 0):
        self.crop_border, self.sse, self.ssim, self.sizes = int(crop_border), [], [], []

    def add(self, pred: torch.Tensor, target: torch.Tensor):
        sse, ssim = restoration_sums(pred, target, self.crop_border)
        if self.sse and self.sse[0].shape[1] != sse.shape[1]:
            raise ValueError(f"a batch of {int(pred.shape[1])} channels after batches with {1 if self.sse[0].shape[1] == 1 else 3}")
        self.sse.append(sse)
        self.ssim.append(ssim)
        self.sizes += [(int(pred.shape[-2]) - 2 * self.crop_border, int(pred.shape[-1]) - 2 * self.crop_border)] * int(sse.shape[0])

    def result(self) -> Dict[str, float]:
        if not self.sse:
            return metrics_from_sums(np.zeros((0, 4, 2), dtype=np.int64), np.zeros((0, 4)), (WINDOW, WINDOW))
        P = int(self.sse[0].shape[1])
        # one copy: the float64 sums travel as their bits next to the integer words
        both = torch.cat([torch.cat(self.sse).reshape(-1, 2 * P), torch.cat(self.ssim).view(torch.int64)], dim=1).cpu().numpy()
        return metrics_from_sums(both[:, :2 * P].reshape(-1, P, 2), both[:, 2 * P:].copy().view(np.float64), np.asarray(self.sizes))
