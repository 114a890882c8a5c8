"""The saliency score restated PER PIXEL in NumPy (the definitions of adm_amd/metrics/saliency.py's docstring): one boolean mask per
threshold, sums over pixels, quadrants as array slices -- no table anywhere.  ``tables_ref`` is the integer table the kernel makes,
through np.bincount.  Shared by tests/test_saliency_host.py, tests/test_hip_saliency_metrics.py and tools/make_golden_saliency.py.
"""
import os

import numpy as np

EPS = 2.0 ** -52
KEYS = ("mae", "max_f", "mean_f", "adp_f", "s_measure", "max_e", "mean_e", "adp_e")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g31_saliency.npz")
REPORT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g31_saliency_report.json")
FAMILIES = ("random", "saturated", "perfect", "inverted", "constant", "narrow", "all_fg", "all_bg", "one_pixel", "soft_block")
HOST_SHAPES = ((1, 1), (1, 7), (5, 1), (7, 13), (33, 65))


def case(family, shape, seed=0):
    """(prediction, map) uint8 [H,W] of one family."""
    H, W = shape
    rng = np.random.default_rng([seed, H, W, FAMILIES.index(family)])
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
    rand = lambda: u8(rng.integers(0, 256, (H, W)))
    blob = np.zeros((H, W), dtype=bool)          # a block off the centre, at least one pixel
    blob[H // 4:max(H // 4 + 1, (3 * H) // 5), W // 3:max(W // 3 + 1, (4 * W) // 5)] = True
    m = u8(blob * 255)
    if family == "random":
        return rand(), rand()
    if family == "saturated":
        return u8((rng.random((H, W)) < 0.4) * 255), u8((rng.random((H, W)) < 0.3) * 255)
    if family == "perfect":
        return m.copy(), m
    if family == "inverted":
        return u8(255 - m), m
    if family == "constant":
        return u8(np.full((H, W), 77)), m
    if family == "narrow":
        return u8(rng.integers(100, 104, (H, W))), m
    if family == "all_fg":
        return rand(), u8(np.full((H, W), 255))
    if family == "all_bg":
        return rand(), u8(np.full((H, W), 128))          # 128 is background: g = [m > 128]
    if family == "one_pixel":
        one = np.zeros((H, W), dtype=np.uint8)
        one[H - 1, W - 1] = 200
        return rand(), one
    if family == "soft_block":
        soft = np.clip(blob * 180.0 + rng.normal(30, 20, (H, W)), 0, 255)
        return u8(np.rint(soft)), m
    raise KeyError(family)


def split_point(g):
    """(cx, cy): the foreground centroid rounded half up in integers, plus one; the middle without foreground."""
    H, W = g.shape
    n_f = int(g.sum())
    if n_f == 0:
        return W // 2 + 1, H // 2 + 1
    ys, xs = np.nonzero(g)
    return (2 * int(xs.sum()) + n_f) // (2 * n_f) + 1, (2 * int(ys.sum()) + n_f) // (2 * n_f) + 1


def tables_ref(p, m):
    """(tables int64 [4,2,256], head int64 [5]) of one pair of uint8 [H,W] planes."""
    p, m = np.asarray(p), np.asarray(m)
    assert p.dtype == np.uint8 and m.dtype == np.uint8 and p.shape == m.shape and p.ndim == 2
    g = m > 128
    cx, cy = split_point(g)
    ys, xs = np.indices(g.shape)
    q = 2 * (ys >= cy) + (xs >= cx)
    key = (q * 2 + g) * 256 + p
    tables = np.bincount(key.reshape(-1), minlength=2048).astype(np.int64).reshape(4, 2, 256)
    head = np.array([g.sum(), (xs * g).sum(), (ys * g).sum(), cx, cy], dtype=np.int64)
    return tables, head


def stretch(p, normalize):
    """(u int64 [H,W], d): the pixel's value is u / d."""
    p = p.astype(np.int64)
    lo, hi = int(p.min()), int(p.max())
    return (p - lo, hi - lo) if normalize and hi > lo else (p, 255)


def f_measure(mask, g):
    tp, fp, n_f = int((mask & g).sum()), int((mask & ~g).sum()), int(g.sum())
    pr, rc = tp / max(tp + fp, 1), tp / max(n_f, 1)
    den = 0.3 * pr + rc
    return 1.3 * pr * rc / den if den != 0 else 0.0


def e_measure(mask, g):
    n, n_f = g.size, int(g.sum())
    if n_f == 0:
        return 1.0 - mask.sum() / n
    if n_f == n:
        return mask.sum() / n
    phi_b, phi_g = mask.astype(np.float64) - mask.sum() / n, g.astype(np.float64) - n_f / n
    a = 2.0 * phi_b * phi_g / (phi_b * phi_b + phi_g * phi_g + EPS)
    return float(((a + 1.0) ** 2 / 4.0).sum() / (n - 1 + EPS))


def _object(x):
    mu = x.mean()
    sigma = x.std(ddof=1) if x.size > 1 else 0.0
    return 2.0 * mu / (mu * mu + 1.0 + sigma + EPS)


def _ssim(u, g, d):
    n = u.size
    su, suu, sg, sug = int(u.sum()), int((u * u).sum()), int(g.sum()), int(u[g].sum())
    vx, vy, cxy = n * suu - su * su, n * sg - sg * sg, n * sug - su * sg
    if su == 0 or sg == 0 or cxy == 0 or n == 1:
        return 1.0 if ((su == 0 and sg == 0) or (vx == 0 and vy == 0) or n == 1) else 0.0
    xm, ym, nn = su / (n * d), sg / n, n * (n - 1)
    sx, sy, sxy = vx / (nn * d * d), vy / nn, cxy / (nn * d)
    return 4.0 * xm * ym * sxy / ((xm * xm + ym * ym) * (sx + sy) + EPS)


def s_measure(u, d, g):
    n, n_f = g.size, int(g.sum())
    s = u / d
    if n_f == 0:
        return 1.0 - s.mean()
    if n_f == n:
        return s.mean()
    s_o = (n_f / n) * _object(s[g]) + ((n - n_f) / n) * _object(1.0 - s[~g])
    cx, cy = split_point(g)
    s_r = 0.0
    for ysl in (slice(0, cy), slice(cy, None)):
        for xsl in (slice(0, cx), slice(cx, None)):
            uq, gq = u[ysl, xsl], g[ysl, xsl]
            if uq.size:
                s_r += (uq.size / n) * _ssim(uq, gq, d)
    return max(0.0, 0.5 * s_o + 0.5 * s_r)


def image_ref(p, m, normalize=True):
    """One pair -> {'mae', 's_measure', 'adp_f', 'adp_e': float; 'f_curve', 'e_curve': float64 [256]}, pixel by pixel."""
    p, m = np.asarray(p), np.asarray(m)
    assert p.dtype == np.uint8 and m.dtype == np.uint8 and p.shape == m.shape and p.ndim == 2
    g = m > 128
    n = g.size
    u, d = stretch(p, normalize)
    b = (255 * u) // d
    masks = [b >= k for k in range(256)]
    adaptive = u * n >= min(2 * int(u.sum()), d * n)
    return {"mae": int(np.abs(u - d * g).sum()) / (d * n), "s_measure": float(s_measure(u, d, g)),
            "adp_f": f_measure(adaptive, g), "adp_e": float(e_measure(adaptive, g)),
            "f_curve": np.array([f_measure(k, g) for k in masks]), "e_curve": np.array([e_measure(k, g) for k in masks], dtype=np.float64)}


def dataset_ref(pairs, normalize=True):
    """[(prediction, map)] -> the eight values of KEYS and ``images``."""
    per = [image_ref(p, m, normalize) for p, m in pairs]
    f, e = np.mean([r["f_curve"] for r in per], axis=0), np.mean([r["e_curve"] for r in per], axis=0)
    mean = lambda k: float(np.mean([r[k] for r in per]))
    return {"mae": mean("mae"), "max_f": float(f.max()), "mean_f": float(f.mean()), "adp_f": mean("adp_f"), "s_measure": mean("s_measure"),
            "max_e": float(e.max()), "mean_e": float(e.mean()), "adp_e": mean("adp_e"), "images": len(per)}


def half_floats():
    """float32 values in (0, 1) whose float32 product with 255 is EXACTLY k + 0.5: a search of the neighbours of (k + 0.5) / 255."""
    out = []
    for k in range(255):
        x = np.float32((k + 0.5) / 255.0)
        cands, lo, hi = [x], x, x
        for _ in range(3):
            lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(1))
            cands += [lo, hi]
        out += [c for c in cands if np.float32(c) * np.float32(255.0) == np.float32(k + 0.5)]
    return np.array(out, dtype=np.float32)
