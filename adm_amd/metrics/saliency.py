"""The saliency score: MAE, maximal / mean / adaptive F-measure (Achanta et al. 2009, beta^2 = 0.3), S-measure (Fan et al. 2017,
alpha = 0.5) and maximal / mean / adaptive E-measure (Fan et al. 2018), the columns of every DUTS-TE table.

Everything is a function of ONE integer table per image.  With prediction bytes p(y, x), map bytes m(y, x), g = [m > 128], N = H W:
  head = (nF, sum x g, sum y g, cx, cy): the foreground count, its 0-based coordinate sums and the split point -- cx = X + 1 with
         X = (2 sum x g + nF) // (2 nF) (the centroid, rounded half up in integers), X = W // 2 when nF = 0; cy likewise;
  T[q][c][v] = the number of pixels with byte v and class c = g in quadrant q = 2 [y >= cy] + [x >= cx].
``saliency_tables`` is one ``adm_saliency_tables`` launch (adm_amd/csrc/saliency_metrics.hip) that makes exactly these, as int64: equal
to a bincount, the same on every run.  ``per_image`` / ``metrics_from_tables`` are the host half, in float64 with eps = 2^-52; every
sum there is an integer sum over at most 256 bins followed by a division, so normalisation costs no pass over the image.

Bins.  hF[v] = sum_q T[q][1][v], hB likewise from class 0, h = hF + hB, nB = N - nF; lo / hi the lowest / highest non-empty bin of h.
With ``normalize`` (the default: the field's evaluation code stretches each prediction to [0, 1]) and hi > lo: u_v = v - lo, d = hi - lo;
otherwise u_v = v, d = 255 -- a constant prediction is not stretched.  Bin v has the value s_v = u_v / d and the threshold bin
b_v = (255 u_v) // d.
  MAE    = (sum hB u + sum hF (d - u)) / (d N)
  curves   for k = 0 .. 255 the binarised prediction is [b_v >= k]: TP_k = sum_{b_v >= k} hF[v], FP_k likewise from hB
  F      : pr = TP / max(TP + FP, 1), rc = TP / max(nF, 1), F = 1.3 pr rc / (0.3 pr + rc), 0 where that denominator is 0
  E      : P = TP + FP.  nF = 0: 1 - P / N.  nF = N: P / N.  Otherwise, over the (bit, truth) combinations (1,1), (1,0), (0,1), (0,0) with
           counts TP, FP, nF - TP, nB - FP:  phi_b = bit - P / N, phi_g = truth - nF / N, a = 2 phi_b phi_g / (phi_b^2 + phi_g^2 + eps),
           E = sum count (a + 1)^2 / 4 / (N - 1 + eps).  A perfect prediction scores N / (N - 1): the definition's known quirk, kept.
  adaptive : the threshold min(2 mean(s), 1), decided in integers: bin v is on where u_v N >= min(2 sum h u, d N); F and E as above.
  S      : nF = 0: 1 - mean(s).  nF = N: mean(s).  Otherwise max(0, 0.5 S_o + 0.5 S_r) with
           S_o = (nF / N) O(s over the foreground) + (nB / N) O(1 - s over the background), O = 2 mu / (mu^2 + 1 + sigma + eps), sigma the
           standard deviation with n - 1 in the denominator (0 for a one-pixel set), and
           S_r = sum_q (n_q / N) ssim_q over the quadrants with n_q > 0.  Per quadrant, in units of u: Su = sum u, Suu = sum u^2, Sg = nF_q,
           Sug = sum_fg u; vx = n Suu - Su^2, vy = n Sg - Sg^2, cxy = n Sug - Su Sg; xm = Su / (n d), ym = Sg / n,
           sx = vx / (n (n-1) d^2), sy = vy / (n (n-1)), sxy = cxy / (n (n-1) d) (all 0 when n = 1); A = 4 xm ym sxy,
           B = (xm^2 + ym^2)(sx + sy); ssim = A / (B + eps) if A != 0, else 1 if B = 0, else 0.  Both zero tests are decided on the
           INTEGERS (A = 0 iff Su = 0 or Sg = 0 or cxy = 0 or n = 1; B = 0 iff Su = Sg = 0 or vx = vy = 0 or n = 1): a float test
           would turn a constant quadrant into noise.
Data set: mae, s_measure, adp_f, adp_e are means over the images; max_f / max_e the maxima over k of the image-MEAN curves (not the
mean of per-image maxima), mean_f / mean_e their means over k; ``images`` the count.

Deviations from common evaluation code: the centroid rounds half up (NumPy rounds half to even); the one-pixel sigma is 0 where
ddof = 1 gives NaN; the weighted F-measure is left out -- it copies the error of the NEAREST foreground pixel, and ties between equally
near pixels make it implementation-defined.
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch

from .. import hip
from ..hip import call, ptr

KEYS = ("mae", "max_f", "mean_f", "adp_f", "s_measure", "max_e", "mean_e", "adp_e")
BINS = 2048          # ADM_SALIENCY_BINS of include/adm_hip.h: 4 quadrants x 2 classes x 256 bytes
MAX_PIXELS = 1 << 24          # ADM_SALIENCY_MAX_PIXELS
EPS = 2.0 ** -52
_V = np.arange(256, dtype=np.int64)


def _plane(t: torch.Tensor, what: str) -> torch.Tensor:
    hip.require_cuda(t, what)
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3:
        raise ValueError(f"{what} must be [B,1,H,W] or [B,H,W], got {tuple(t.shape)}")
    return t.contiguous()


@torch.no_grad()
def saliency_tables(pred: torch.Tensor, gt_u8: torch.Tensor):
    """pred uint8 or float32 (in [0, 1]; quantised in the kernel as the samplers' PNG writer does) and gt_u8 uint8, both [B,1,H,W] or
    [B,H,W] on the GPU -> (tables int64 [B,4,2,256], head int64 [B,5]) on the GPU."""
    pred, gt_u8 = _plane(pred, "the prediction"), _plane(gt_u8, "the map")
    if pred.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"the prediction must be uint8 or float32, got {pred.dtype}")
    if gt_u8.dtype != torch.uint8:
        raise ValueError(f"the map must be uint8 (its bytes, foreground = byte > 128), got {gt_u8.dtype}")
    if pred.shape != gt_u8.shape:
        raise ValueError(f"the prediction and the map differ in shape: {tuple(pred.shape)} and {tuple(gt_u8.shape)}")
    B, H, W = (int(v) for v in pred.shape)
    if not 1 <= B <= 65535 or H < 1 or W < 1 or H * W > MAX_PIXELS:
        raise ValueError(f"saliency_tables takes 1 .. 65535 images of 1 .. 2^24 pixels, got {B} of {H}x{W}")
    tables = torch.empty(B, 4, 2, 256, device=pred.device, dtype=torch.int64)
    head = torch.empty(B, 5, device=pred.device, dtype=torch.int64)
    call("adm_saliency_tables", ptr(pred), int(pred.dtype == torch.float32), ptr(gt_u8), ptr(tables), ptr(head), B, H, W)
    return tables, head


def _f_measure(tp, fp, n_f: int):
    pr = tp / np.maximum(tp + fp, 1)
    rc = tp / max(n_f, 1)
    den = 0.3 * pr + rc
    return np.where(den != 0, 1.3 * pr * rc / np.where(den != 0, den, 1.0), 0.0)


def _e_measure(tp, fp, n_f: int, n: int):
    p = (tp + fp) / n
    if n_f == 0:
        return 1.0 - p
    if n_f == n:
        return p
    total = np.zeros(np.shape(p))
    for bit, truth, count in ((1, 1, tp), (1, 0, fp), (0, 1, n_f - tp), (0, 0, (n - n_f) - fp)):
        phi_b, phi_g = bit - p, truth - n_f / n
        a = 2.0 * phi_b * phi_g / (phi_b * phi_b + phi_g * phi_g + EPS)
        total = total + count * ((a + 1.0) ** 2 / 4.0)
    return total / (n - 1 + EPS)


def _object(hist, u, d: int, n: int):
    """O of the values u / d counted by hist (n = its sum > 0): 2 mu / (mu^2 + 1 + sigma + eps)."""
    su, suu = int((hist * u).sum()), int((hist * u * u).sum())
    mu = su / (n * d)
    sigma = math.sqrt((n * suu - su * su) / (n * (n - 1))) / d if n > 1 else 0.0
    return 2.0 * mu / (mu * mu + 1.0 + sigma + EPS)


def _ssim(t_q, u, d: int):
    """(n, ssim) of one quadrant's table [2][256]."""
    h_q = t_q[0] + t_q[1]
    n = int(h_q.sum())
    if n == 0:
        return 0, 0.0
    su, suu, sg, sug = int((h_q * u).sum()), int((h_q * u * u).sum()), int(t_q[1].sum()), int((t_q[1] * u).sum())
    vx, vy, cxy = n * suu - su * su, n * sg - sg * sg, n * sug - su * sg
    a_zero = su == 0 or sg == 0 or cxy == 0 or n == 1
    b_zero = (su == 0 and sg == 0) or (vx == 0 and vy == 0) or n == 1
    if a_zero:
        return n, 1.0 if b_zero else 0.0
    xm, ym, nn = su / (n * d), sg / n, n * (n - 1)
    sx, sy, sxy = vx / (nn * d * d), vy / nn, cxy / (nn * d)
    return n, 4.0 * xm * ym * sxy / ((xm * xm + ym * ym) * (sx + sy) + EPS)


def _one(t, normalize: bool):
    """One image's table int64 [4][2][256] -> (mae, s_measure, adp_f, adp_e, F curve [256], E curve [256])."""
    h_f, h_b = t[:, 1].sum(0), t[:, 0].sum(0)
    h = h_f + h_b
    n_f, n = int(h_f.sum()), int(h.sum())
    filled = np.nonzero(h)[0]
    lo, hi = int(filled[0]), int(filled[-1])
    u, d = (_V - lo, hi - lo) if normalize and hi > lo else (_V, 255)
    su = int((h * u).sum())
    mae = (int((h_b * u).sum()) + int((h_f * (d - u)).sum())) / (d * n)
    # the curves: counts per threshold bin, then sums over b_v >= k
    b = np.clip((255 * u) // d, 0, 255)          # (only empty bins are clipped)
    tp_bins, fp_bins = np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)
    np.add.at(tp_bins, b, h_f)
    np.add.at(fp_bins, b, h_b)
    tp, fp = np.cumsum(tp_bins[::-1])[::-1], np.cumsum(fp_bins[::-1])[::-1]
    f_curve, e_curve = _f_measure(tp, fp, n_f), _e_measure(tp, fp, n_f, n)
    # the adaptive threshold min(2 mean(s), 1), in integers
    on = (u * n >= min(2 * su, d * n)) & (h > 0)
    tp_a, fp_a = np.asarray(int(h_f[on].sum())), np.asarray(int(h_b[on].sum()))
    adp_f, adp_e = float(_f_measure(tp_a, fp_a, n_f)), float(_e_measure(tp_a, fp_a, n_f, n))
    mean_s = su / (d * n)
    if n_f == 0:
        s = 1.0 - mean_s
    elif n_f == n:
        s = mean_s
    else:
        s_o = (n_f / n) * _object(h_f, u, d, n_f) + ((n - n_f) / n) * _object(h_b, d - u, d, n - n_f)
        s_r = 0.0
        for q in range(4):
            n_q, ssim = _ssim(t[q], u, d)
            s_r += (n_q / n) * ssim
        s = max(0.0, 0.5 * s_o + 0.5 * s_r)
    return mae, s, adp_f, adp_e, f_curve, e_curve


def per_image(tables, head, hw, normalize: bool = True) -> Dict[str, np.ndarray]:
    """tables int64 [n,4,2,256], head int64 [n,5], hw = (H, W) or [n,2] -> {'mae', 's_measure', 'adp_f', 'adp_e': float64 [n];
    'f_curve', 'e_curve': float64 [n,256]}.  A table whose sum is not H W, or whose foreground is not head's nF, raises."""
    t = np.asarray(tables, dtype=np.int64).reshape(-1, 4, 2, 256)
    hd = np.asarray(head, dtype=np.int64).reshape(-1, 5)
    n = t.shape[0]
    sizes = np.broadcast_to(np.asarray(hw, dtype=np.int64).reshape(-1, 2), (n, 2))
    if hd.shape[0] != n:
        raise ValueError(f"{n} tables but {hd.shape[0]} heads")
    out = {k: np.zeros(n) for k in ("mae", "s_measure", "adp_f", "adp_e")}
    out["f_curve"], out["e_curve"] = np.zeros((n, 256)), np.zeros((n, 256))
    for i in range(n):
        H, W = int(sizes[i, 0]), int(sizes[i, 1])
        if int(t[i].sum()) != H * W or int(t[i, :, 1].sum()) != int(hd[i, 0]) or (t[i] < 0).any():
            raise ValueError(f"image {i}: its table counts {int(t[i].sum())} pixels, {int(t[i, :, 1].sum())} of them foreground; "
                             f"expected {H}x{W} = {H * W} and head's nF = {int(hd[i, 0])}")
        out["mae"][i], out["s_measure"][i], out["adp_f"][i], out["adp_e"][i], out["f_curve"][i], out["e_curve"][i] = _one(t[i], normalize)
    return out


def metrics_from_tables(tables, head, hw, normalize: bool = True) -> Dict[str, float]:
    """The eight values of ``KEYS`` over the data set, plus ``images``; NaN without an image."""
    m = per_image(tables, head, hw, normalize)
    n = int(m["mae"].shape[0])
    if n == 0:
        return dict({k: math.nan for k in KEYS}, images=0)
    f, e = m["f_curve"].mean(0), m["e_curve"].mean(0)
    return {"mae": float(m["mae"].mean()), "max_f": float(f.max()), "mean_f": float(f.mean()), "adp_f": float(m["adp_f"].mean()),
            "s_measure": float(m["s_measure"].mean()), "max_e": float(e.max()), "mean_e": float(e.mean()),
            "adp_e": float(m["adp_e"].mean()), "images": n}


class SaliencyScore:
    """Accumulates ``saliency_tables`` of batches on the device; ``result()`` makes the one host copy."""

    def __init__(self, normalize: bool = True):
        self.normalize, self.tables, self.heads, self.sizes = bool(normalize), [], [], []

    def add(self, pred: torch.Tensor, gt_u8: torch.Tensor):
        tables, head = saliency_tables(pred, gt_u8)
        self.tables.append(tables)
        self.heads.append(head)
        self.sizes += [(int(pred.shape[-2]), int(pred.shape[-1]))] * int(tables.shape[0])

    def result(self) -> Dict[str, float]:
        if not self.tables:
            return metrics_from_tables(np.zeros((0, 4, 2, 256), dtype=np.int64), np.zeros((0, 5), dtype=np.int64), (1, 1), self.normalize)
        both = torch.cat([torch.cat(self.tables).reshape(-1, BINS), torch.cat(self.heads)], dim=1).cpu().numpy()
        return metrics_from_tables(both[:, :BINS], both[:, BINS:], np.asarray(self.sizes), self.normalize)
