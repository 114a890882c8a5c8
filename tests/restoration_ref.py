"""The restoration score restated per image in NumPy float64 (the definitions of adm_amd/metrics/restoration.py's docstring): the
DIRECT 11 x 11 window -- 121 shifted slices times the outer-product weights, never the two 1-D passes the kernel makes --, Python
integers for the squared-error sums.  ``ssim_scipy`` is the same map through scipy.signal.convolve2d(..., 'valid');
``ssim_separable`` is the kernel's own arithmetic (rows, then columns) in a chosen dtype: float64 to show the two orders agree, float32
to show what the bar is there to reject.  Shared by tests/test_restoration_host.py, tests/test_hip_restoration_metrics.py,
tools/make_golden_restoration.py and tools/restoration_metrics_cost.py.
"""
import math
import os

import numpy as np

KEYS = ("psnr", "ssim", "psnr_y", "ssim_y")
K, SIGMA, C1, C2 = 11, 1.5, 6.5025, 58.5225
Y_SCALE = 255000
BAR = 1e-10          # per-plane SSIM, absolute (tests/test_hip_restoration_metrics.py derives it)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g32_restoration.npz")
REPORT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g32_restoration_report.json")
FAMILIES = ("uniform", "saturated", "equal", "flat", "noise", "fringe")
TILE = 32          # ADM_RESTORATION_TILE
# the GPU tests' shapes, (H', W') after the shave and B: one valid position; one over in either axis; one tile exactly; one position over
# / under; 2 x 3 tiles with ragged edges; odd sizes in a batch of three, so that images start off every 16-byte boundary
GPU_SHAPES = [((11, 11), 1), ((11, 12), 1), ((12, 11), 2), ((TILE + 10, TILE + 10), 1), ((TILE + 11, TILE + 9), 1),
              ((TILE + 23, 2 * TILE + 23), 1), ((13, 17), 3)]


def window1d():
    x = np.arange(K, dtype=np.float64) - (K - 1) / 2
    w = np.exp(-(x * x) / (2.0 * SIGMA * SIGMA))
    return w / w.sum()


def window2d():
    w = window1d()
    return np.outer(w, w)


def quantise(v):
    """uint8 of a float array in [0, 1] by the kernel's rule: rint(clip(v, 0, 1) * 255) in float32, ties to even, NaN -> 0."""
    v = np.asarray(v, dtype=np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.rint(np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)


def case(family, shape, channels=3, seed=0):
    """(prediction, target) uint8 [C,H,W] of one family."""
    H, W = shape
    rng = np.random.default_rng([seed, H, W, channels, FAMILIES.index(family)])
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
    rand = lambda: u8(rng.integers(0, 256, (channels, H, W)))
    if family == "uniform":
        return rand(), rand()
    if family == "saturated":
        return u8((rng.random((channels, H, W)) < 0.5) * 255), u8((rng.random((channels, H, W)) < 0.5) * 255)
    if family == "equal":
        g = rand()
        return g.copy(), g
    if family == "flat":          # 255 against 254: w*x^2 - mu^2 cancels at magnitude 65025 against C2 = 58.5
        return u8(np.full((channels, H, W), 255)), u8(np.full((channels, H, W), 254))
    if family == "noise":
        g = rand()
        return u8(np.clip(g.astype(np.int64) + rng.integers(-3, 4, g.shape), 0, 255)), g
    if family == "fringe":          # equal but for the last 10 rows, the last 10 columns and the corner: what finds an unowned pixel
        g = rand()
        p = g.copy()
        p[:, H - 10:, :] = 255 - g[:, H - 10:, :]
        p[:, :, W - 10:] = 255 - g[:, :, W - 10:]
        return p, g
    raise KeyError(family)


def shave(x, s):
    return x[..., s:x.shape[-2] - s, s:x.shape[-1] - s] if s else x


def planes(x):
    """uint8 [C,H,W] -> (values float64 [P,H,W], integers int64 [P,H,W], scale per plane): R, G, B, Y for C = 3, else the plane."""
    i = x.astype(np.int64)
    if x.shape[0] == 1:
        return i.astype(np.float64), i, [1]
    n = 65481 * i[0] + 128553 * i[1] + 24966 * i[2]
    values = np.concatenate([i.astype(np.float64), (16.0 + n.astype(np.float64) / 255000.0)[None]])
    return values, np.concatenate([i, n[None]]), [1, 1, 1, Y_SCALE]


def ssim_map(p, g):
    """The SSIM map of two float64 planes [H,W] over the valid positions, with the direct 2-D window."""
    w2 = window2d()
    Hv, Wv = p.shape[0] - K + 1, p.shape[1] - K + 1
    mp, mg, pp, gg, pg = (np.zeros((Hv, Wv)) for _ in range(5))
    for i in range(K):
        for j in range(K):
            a, b, w = p[i:i + Hv, j:j + Wv], g[i:i + Hv, j:j + Wv], w2[i, j]
            mp += w * a
            mg += w * b
            pp += w * (a * a)
            gg += w * (b * b)
            pg += w * (a * b)
    return _ssim_value(mp, mg, pp, gg, pg)


def _ssim_value(mp, mg, pp, gg, pg):
    vp, vg, cov = pp - mp * mp, gg - mg * mg, pg - mp * mg
    return ((2 * (mp * mg) + C1) * (2 * cov + C2)) / ((mp * mp + mg * mg + C1) * (vp + vg + C2))


def ssim_scipy(p, g):
    """The same map through scipy.signal.convolve2d (the window is symmetric, so convolution is correlation)."""
    from scipy.signal import convolve2d
    w2 = window2d()
    f = lambda x: convolve2d(x, w2, mode="valid")
    return _ssim_value(f(p), f(g), f(p * p), f(g * g), f(p * g))


def ssim_separable(p, g, dtype=np.float64):
    """The kernel's order of operations -- 11 taps along x, then 11 along y -- in `dtype`."""
    w = window1d().astype(dtype)
    p, g = p.astype(dtype), g.astype(dtype)
    Hv, Wv = p.shape[0] - K + 1, p.shape[1] - K + 1

    def f(x):
        rows = np.zeros((x.shape[0], Wv), dtype=dtype)
        for k in range(K):
            rows += w[k] * x[:, k:k + Wv]
        out = np.zeros((Hv, Wv), dtype=dtype)
        for k in range(K):
            out += w[k] * rows[k:k + Hv]
        return out

    c1, c2 = dtype(C1), dtype(C2)
    mp, mg, pp, gg, pg = f(p), f(g), f(p * p), f(g * g), f(p * g)
    vp, vg, cov = pp - mp * mp, gg - mg * mg, pg - mp * mg
    return ((dtype(2) * (mp * mg) + c1) * (dtype(2) * cov + c2)) / ((mp * mp + mg * mg + c1) * (vp + vg + c2))


def psnr_of(sse, count, scale=1):
    return math.inf if sse == 0 else 10.0 * math.log10((255 * 255 * scale * scale * count) / sse)


def image_ref(pred, target, crop_border=0, ssim=ssim_map):
    """uint8 [C,H,W] pair -> {'sse': [P] Python integers, 'ssim_planes': float64 [P], 'psnr', 'ssim' (+ 'psnr_y', 'ssim_y' for C = 3)}."""
    p, g = shave(np.asarray(pred), crop_border), shave(np.asarray(target), crop_border)
    assert p.dtype == np.uint8 and g.dtype == np.uint8 and p.shape == g.shape and p.shape[0] in (1, 3)
    (pv, pi, scale), (gv, gi, _) = planes(p), planes(g)
    H, W = p.shape[-2:]
    sse = [sum(np.square(pi[k] - gi[k]).ravel().tolist()) for k in range(len(scale))]          # (each square < 2^52: exact in int64; the SUM is Python's)
    per = np.array([float(ssim(pv[k], gv[k]).mean()) for k in range(len(scale))])
    rgb = 3 if len(scale) == 4 else 1
    out = {"sse": sse, "ssim_planes": per, "psnr": psnr_of(sum(sse[:rgb]), rgb * H * W), "ssim": float(per[:rgb].mean())}
    if rgb == 3:
        out["psnr_y"], out["ssim_y"] = psnr_of(sse[3], H * W, Y_SCALE), float(per[3])
    return out


_batches = {}


def batch_ref(family, hw, B, C, s):
    """(pred, target) uint8 [B,C,H' + 2s,W' + 2s], read-only, and the per-image restatement: computed once, shared, never changed."""
    key = (family, hw, B, C, s)
    if key not in _batches:
        pairs = [case(family, (hw[0] + 2 * s, hw[1] + 2 * s), C, seed=b) for b in range(B)]
        p, g = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
        p.setflags(write=False), g.setflags(write=False)
        _batches[key] = (p, g, [image_ref(a, b, s) for a, b in pairs])
    return _batches[key]


def words(sse):
    """Python integers [P] -> int64 [P,2] of {lo, hi}."""
    return np.array([[v & 0xffffffff, v >> 32] for v in sse], dtype=np.int64)


def dataset_ref(pairs, crop_border=0):
    """The mean over the images of every metric, plus ``images``."""
    per = [image_ref(p, g, crop_border) for p, g in pairs]
    keys = [k for k in KEYS if k in per[0]]
    return dict({k: float(np.mean([r[k] for r in per])) for k in keys}, images=len(per))
