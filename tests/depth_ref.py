"""NumPy restatement of the depth recipe's batch (ddm.data.NYUDv2DepthDataset.__getitem__, ddm/data.py:869-887 of the reference) and
of its score, for the tests: slicing for the box, the crop and the flip, float32 for the two value maps, float64 for the metrics.
tests/golden/g29_depth_data.npz (tools/make_golden_depth.py) holds what PIL itself makes of the same sources."""
import hashlib

import numpy as np

F = np.float32
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "silog", "log10", "d1", "d2", "d3")


def hash_values(shape, tag, high):
    """Deterministic integers in [0, high) of the given shape (SHA-256 counter mode), as int64."""
    n = int(np.prod(shape))
    out = np.empty(n, dtype=np.int64)
    raw = b"".join(hashlib.sha256(f"{tag}:{i}".encode()).digest() for i in range((4 * n + 31) // 32))
    words = np.frombuffer(raw, dtype="<u4")[:n].astype(np.int64)
    out[:] = words % int(high)
    return out.reshape(shape)


def crop(plane, box, top, left, size, flip):
    """The boxed frame's (top, left) crop of ``size`` = (H, W), mirrored along the columns when ``flip``: PIL's .crop(box), the
    RandomCrop's .crop and .transpose(FLIP_LEFT_RIGHT) as slices.  box = PIL's (left, upper, right, lower)."""
    bl, bu, br, bb = box
    frame = plane[bu:bb, bl:br]
    H, W = size
    assert 0 <= top <= frame.shape[0] - H and 0 <= left <= frame.shape[1] - W, (frame.shape, top, left, size)
    out = frame[top:top + H, left:left + W]
    return np.ascontiguousarray(out[:, ::-1] if flip else out)


def depth_to_float(d):
    """uint16 [...] -> float32: float32(depth) / 10000 * 2 - 1, unclipped (data.py:880-886)."""
    return (d.astype(F) / F(10000)) * F(2) - F(1)


def photo_to_float(u8):
    """uint8 [..., H, W, 3] -> float32 [..., 3, H, W]: to_tensor * 2 - 1 (data.py:879, 885)."""
    return np.ascontiguousarray(np.moveaxis((u8.astype(F) / F(255)) * F(2) - F(1), -1, -3))


def batch(photos, depths, box, idx, top, left, flip, size):
    """(image float32 [B,1,H,W], cond float32 [B,3,H,W]) of the draws."""
    image = np.stack([depth_to_float(crop(depths[i], box, t, l, size, f))[None] for i, t, l, f in zip(idx, top, left, flip)])
    cond = np.stack([photo_to_float(crop(photos[i], box, t, l, size, f)) for i, t, l, f in zip(idx, top, left, flip)])
    return image, cond


def ratios(pred, gt, min_depth=1e-3, max_depth=10.0):
    """max(p/g, g/p) in float64 over the valid pixels of pred / gt (depth fractions of 10 m), flattened."""
    g = gt.astype(np.float64).reshape(-1) * 10.0
    p = np.clip(pred.astype(np.float64).reshape(-1) * 10.0, min_depth, max_depth)
    ok = (g > min_depth) & (g < max_depth)
    return np.maximum(p[ok] / g[ok], g[ok] / p[ok])


def sums(pred, gt, min_depth=1e-3, max_depth=10.0):
    """float64 [B, 10] of pred / gt float32 [B,1,H,W]: {n, S|p-g|/g, S(p-g)^2/g, S(p-g)^2, S(ln p - ln g)^2, S(ln p - ln g),
    S|log10 p - log10 g|, #[r < 1.25], #[r < 1.25^2], #[r < 1.25^3]} over min_depth < g < max_depth, p clamped to the range."""
    out = np.zeros((pred.shape[0], 10), dtype=np.float64)
    for b in range(pred.shape[0]):
        g = gt[b].astype(np.float64).reshape(-1) * 10.0
        p = np.clip(pred[b].astype(np.float64).reshape(-1) * 10.0, min_depth, max_depth)
        ok = (g > min_depth) & (g < max_depth)
        g, p = g[ok], p[ok]
        if g.size == 0:
            continue
        d, dl, r = p - g, np.log(p) - np.log(g), np.maximum(p / g, g / p)
        out[b] = [g.size, (np.abs(d) / g).sum(), (d * d / g).sum(), (d * d).sum(), (dl * dl).sum(), dl.sum(),
                  np.abs(np.log10(p) - np.log10(g)).sum()] + [float((r < t).sum()) for t in THRESHOLDS]
    return out


def metrics(s):
    """{key: mean over the images with a valid pixel} + images / skipped, from float64 [B, 10] sums."""
    rows = []
    for n, a, sq, se, l2, l1, lg, d1, d2, d3 in np.asarray(s, dtype=np.float64).reshape(-1, 10):
        if n > 0:
            rows.append([a / n, sq / n, np.sqrt(se / n), np.sqrt(l2 / n), 100.0 * np.sqrt(max(l2 / n - (l1 / n) ** 2, 0.0)), lg / n,
                         d1 / n, d2 / n, d3 / n])
    res = {k: float(np.mean([r[i] for r in rows])) if rows else float("nan") for i, k in enumerate(KEYS)}
    res["images"], res["skipped"] = len(rows), len(s) - len(rows)
    return res


def nyud_tree(root, frames=((30, 40), (30, 40), (33, 41))):
    """A small NYUv2-shaped tree written with PIL: train/ with two pairs in scene folders, test/ with one; pair i is ``rgb_0000i.jpg``
    (hash bytes 'tree.p{i}', lossy) + ``sync_depth_0000i.png`` (16 bits, hash values 'tree.d{i}' in [0, 10000])."""
    from PIL import Image
    layout = {"train": [("kitchen_0001", 0), ("office_0002", 1)], "test": [("bathroom", 2)]}
    for split, scenes in layout.items():
        for scene, i in scenes:
            folder = root / split / scene
            folder.mkdir(parents=True)
            h, w = frames[i]
            Image.fromarray(hash_values((h, w, 3), f"tree.p{i}", 256).astype(np.uint8)).save(folder / f"rgb_{i:05d}.jpg")
            Image.fromarray(hash_values((h, w), f"tree.d{i}", 10001).astype(np.uint16)).save(folder / f"sync_depth_{i:05d}.png")
    return layout
