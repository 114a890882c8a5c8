#!/usr/bin/env python3
"""Writes tests/golden/g29_depth_data.npz (CPU): what PIL itself makes of small depth pairs under the item sequence of
ddm.data.NYUDv2DepthDataset (ddm/data.py:869-887 of the reference).

Two ragged pairs -- a 16-bit png of raw depths and a jpg photo each -- are written to a temporary folder and read back as the dataset
reads them: ``Image.open(photo).convert('RGB')`` / ``Image.open(depth)`` (mode I;16), ``.crop(box)`` of both, then per scripted draw
the RandomCrop's ``.crop((left, top, left + W, top + H))`` and, when flipped, ``.transpose(FLIP_LEFT_RIGHT)``, and ``np.array``.
torchvision is not needed: RandomCrop and RandomHorizontalFlip on PIL images are exactly those two calls with drawn arguments, and
the draws here are scripted.  The reference's module is not imported.

Recorded: the sources as decoded (``photo{i}`` uint8 [h,w,3] -- jpg is lossy, so the decoded bytes are the source --, ``depth{i}``
uint16 [h,w]), ``box``, ``cases`` int32 [K, 7] = (pair, top, left, flip, H, W, whole) and PIL's outputs ``out_photo{k}`` uint8
[H,W,3] / ``out_depth{k}`` uint16 [H,W].  ``whole`` = 1: the test-split item, the boxed frame itself (no crop, no flip).
"""
import os
import sys
import tempfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import depth_ref as R  # noqa: E402

SIZES = [(23, 29), (27, 35)]
BOX = (3, 2, 27, 21)          # PIL's (left, upper, right, lower): a 19 x 24 frame; the left edge is odd
SPECIAL = (0, 1, 9999, 10000, 65535)
# (pair, top, left, flip, H, W): offsets at 0 and at their maxima, odd lefts, both flips, a repeated pair; W = 18 is no multiple of 4
CROPS = [(0, 0, 0, 0, 16, 20), (1, 3, 4, 1, 16, 20), (1, 0, 3, 0, 16, 20), (0, 3, 1, 1, 16, 20), (1, 3, 4, 0, 16, 20),
         (0, 0, 0, 1, 15, 18), (1, 4, 6, 0, 15, 18), (0, 4, 5, 1, 15, 18), (0, 2, 6, 0, 15, 18), (1, 1, 1, 1, 15, 18)]


def sources():
    photos, depths = [], []
    for i, (h, w) in enumerate(SIZES):
        photos.append(R.hash_values((h, w, 3), f"g29.photo{i}", 256).astype(np.uint8))
        d = R.hash_values((h, w), f"g29.depth{i}", 10001).astype(np.uint16)
        # the special values inside the box, on its edges and corners
        bl, bu, br, bb = BOX
        spots = [(bu, bl), (bu, br - 1), (bb - 1, bl), (bb - 1, br - 1), (bu + 7, bl + 9), (bu + 3, bl + 1), (bb - 2, br - 3)]
        for k, (y, x) in enumerate(spots):
            d[y, x] = SPECIAL[(k + i) % len(SPECIAL)]
        depths.append(d)
    return photos, depths


def main():
    photos, depths = sources()
    out = {"box": np.asarray(BOX, dtype=np.int32)}
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        opened = []
        for i, (p, d) in enumerate(zip(photos, depths)):
            pp, dp = os.path.join(tmp, f"rgb_{i:05d}.jpg"), os.path.join(tmp, f"sync_depth_{i:05d}.png")
            Image.fromarray(p).save(pp, quality=92)
            Image.fromarray(d).save(dp)
            rgb, depth = Image.open(pp).convert("RGB"), Image.open(dp)
            assert depth.mode == "I;16", depth.mode
            out[f"photo{i}"], out[f"depth{i}"] = np.array(rgb), np.array(depth)
            assert out[f"depth{i}"].dtype == np.uint16 and np.array_equal(out[f"depth{i}"], d)
            opened.append((rgb.crop(BOX), depth.crop(BOX)))          # data.py:875-876
        k = 0
        for i in range(len(SIZES)):          # split: test -- the boxed frame itself
            rgb, depth = opened[i]
            out[f"out_photo{k}"], out[f"out_depth{k}"] = np.array(rgb), np.array(depth)
            cases.append((i, 0, 0, 0, depth.size[1], depth.size[0], 1))
            k += 1
        for i, top, left, flip, H, W in CROPS:          # split: train -- RandomCrop's crop, RandomHorizontalFlip's transpose
            rgb, depth = (im.crop((left, top, left + W, top + H)) for im in opened[i])
            if flip:
                rgb, depth = (im.transpose(Image.FLIP_LEFT_RIGHT) for im in (rgb, depth))
            out[f"out_photo{k}"], out[f"out_depth{k}"] = np.array(rgb), np.array(depth)
            assert out[f"out_depth{k}"].dtype == np.uint16 and out[f"out_depth{k}"].shape == (H, W)
            cases.append((i, top, left, flip, H, W, 0))
            k += 1
    out["cases"] = np.asarray(cases, dtype=np.int32)
    path = os.path.join(ROOT, "tests", "golden", "g29_depth_data.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cases)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
