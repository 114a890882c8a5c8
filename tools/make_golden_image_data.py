#!/usr/bin/env python3
"""Golden vectors for the one-plane first-stage batches (adm_image_resize_batch): PIL's own bytes.  Needs PIL only (no GPU, no
reference import: ddm.data needs torchvision, which is not a dependency here).  The steps of ddm.data.ImageDataset.__getitem__
(data.py:167-185 of the reference; the map of DUTSDataset and the photo of SketchDataset go through the same ones) are performed
with the PIL operations torchvision's PIL path resolves to, in the reference's order:
  data.py:180   Image.open(..).convert("RGB") (or "L")          -> Image.fromarray of a uint8 [h,w,3] / [h,w] array
  data.py:169   Resize(image_size): F.resize(img, [H, W], BILINEAR)   -> img.resize((W, H), Image.BILINEAR)
  data.py:170   RandomHorizontalFlip: F.hflip                  -> img.transpose(Image.FLIP_LEFT_RIGHT), draw given
Writes tests/golden/g28_image_data.npz (below 200 KB): for C = 1 and C = 3 the source bytes of every image of the pool and, per
target, PIL's resized bytes unflipped and flipped.

Sources (height x width).  C = 1: 29x37, 30x38, 31x39, 32x40 (rows of 37..40 bytes: all four row-start residues mod 4 occur, in
every image and at the images' own starts), a 33x1 source ONE PIXEL WIDE, and a last 9x11 image after which the pool ends off a
dword boundary.  C = 3: 20x24 (up-scaling), 32x32 (the identity at the 32x32 target), 103x99 (about 3.2x down), and a last 7x6 image
after which the pool ends off a dword boundary.  Targets: 32x32, 48x32 and 40x24 (ragged 16x16 tiles in both axes)."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sr_data_ref import hash_bytes  # noqa: E402

SOURCES = {1: [(29, 37), (30, 38), (31, 39), (32, 40), (33, 1), (9, 11)], 3: [(20, 24), (32, 32), (103, 99), (7, 6)]}
TARGETS = [(32, 32), (48, 32), (40, 24)]


def item(img, out_hw, flip):
    H, W = out_hw
    im = Image.fromarray(img)
    assert im.mode == ("RGB" if img.ndim == 3 else "L")
    im = im.resize((W, H), Image.BILINEAR)          # PIL sizes are (width, height)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im)


g = {"pil_version": np.array(PIL.__version__), "targets": np.array(TARGETS, dtype=np.int32)}
for C, sizes in SOURCES.items():
    g[f"c{C}.sizes"] = np.array(sizes, dtype=np.int32)
    total = 0
    for i, (h, w) in enumerate(sizes):
        src = hash_bytes((h, w, 3) if C == 3 else (h, w), f"image_data.c{C}.s{i}")
        total += src.size
        g[f"c{C}.s{i}.src"] = src
        for H, W in TARGETS:
            g[f"c{C}.s{i}.t{H}x{W}"] = item(src, (H, W), False)
            g[f"c{C}.s{i}.t{H}x{W}.flipped"] = item(src, (H, W), True)
    assert total % 4 != 0, f"C = {C}: the pool's bytes end on a dword boundary ({total})"
starts = np.cumsum([0] + [h * w for h, w in SOURCES[1]])[:-1]
residues = {int((s + r * w) % 4) for s, (h, w) in zip(starts, SOURCES[1][:4]) for r in range(h)}
assert residues == {0, 1, 2, 3}, residues

out = os.path.join(ROOT, "tests", "golden", "g28_image_data.npz")
np.savez_compressed(out, **g)
size = os.path.getsize(out)
assert size < 200 * 1000, size
print(f"wrote {out}: {len(g)} arrays, {size} bytes, PIL {PIL.__version__}")
