#!/usr/bin/env python3
"""Golden vectors for the saliency pairs: PIL's own bytes.  Needs PIL only (no GPU, no reference import: ddm.data needs torchvision,
which is not a dependency here).  The steps of ddm.data.DUTSDataset.__getitem__ are performed with the PIL operations torchvision's
PIL path resolves to, in the reference's order:
  data.py:1002-1004   Image.open(..).convert("RGB") / .convert("L")            -> Image.fromarray of a uint8 [h,w,3] / [h,w] array
  data.py:983, 1144   Resize(image_size): F.resize(img, [H, W], BILINEAR)      -> img.resize((W, H), Image.BILINEAR), photo and map
                      each from ITS OWN size (:1145, interpolation2 defaults to the same filter)
  data.py:984, 1158   RandomHorizontalFlip: F.hflip of both on one draw        -> img.transpose(Image.FLIP_LEFT_RIGHT), draw given
Writes tests/golden/g23_duts_data.npz: per case of tests/duts_data_ref.CASES the checksum of its hashed sources and PIL's resized
bytes (the sources themselves are regenerated from their tags), the flipped outputs the batch of DRAWS needs, and one small
high-contrast source on which a resize without PIL's uint8 intermediate gives other bytes, with PIL's outputs for it."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import duts_data_ref as R  # noqa: E402


def duts_item(photo, gmap, out_hw, flip):
    H, W = out_hw
    rgb = Image.fromarray(photo).resize((W, H), Image.BILINEAR)          # PIL sizes are (width, height)
    gt = Image.fromarray(gmap).resize((W, H), Image.BILINEAR)
    assert rgb.mode == "RGB" and gt.mode == "L"
    if flip:
        rgb, gt = rgb.transpose(Image.FLIP_LEFT_RIGHT), gt.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(rgb), np.asarray(gt)


g = {"pil_version": np.array(PIL.__version__), "target": np.array(R.TARGET, dtype=np.int32),
     "sizes": np.array(R.CASES, dtype=np.int32), "draws": np.array(R.DRAWS, dtype=np.int32)}
for i in range(len(R.CASES)):
    photo, gmap = R.case_sources(i)
    g[f"c{i}.checksum"] = np.array([int(photo.astype(np.int64).sum()), int(gmap.astype(np.int64).sum())], dtype=np.int64)
    g[f"c{i}.rgb"], g[f"c{i}.gray"] = duts_item(photo, gmap, R.TARGET, False)
for i in sorted({i for i, f in R.DRAWS if f}):
    g[f"c{i}.rgb_flipped"], g[f"c{i}.gray_flipped"] = duts_item(*R.case_sources(i), R.TARGET, True)

# the uint8 intermediate: 0 / 255 bytes, 29x45 -> 16x24; keep the first seed on which rounding once differs from PIL in BOTH planes
for seed in range(64):
    rng = np.random.RandomState(seed)
    photo = (rng.randint(0, 2, (29, 45, 3)) * 255).astype(np.uint8)
    gmap = (rng.randint(0, 2, (31, 41)) * 255).astype(np.uint8)
    rgb, gray = duts_item(photo, gmap, (16, 24), False)
    d_rgb = int((R.resize_rounded_once(photo, (16, 24)) != rgb).sum())
    d_gray = int((R.resize_rounded_once(np.repeat(gmap[:, :, None], 3, axis=2), (16, 24))[:, :, 0] != gray).sum())
    if d_rgb > 0 and d_gray > 0:
        break
else:
    raise SystemExit("no seed separates the uint8 intermediate from a single rounding")
g["edge.photo"], g["edge.map"], g["edge.rgb"], g["edge.gray"] = photo, gmap, rgb, gray
g["edge.differing"] = np.array([d_rgb, d_gray], dtype=np.int32)

out = os.path.join(ROOT, "tests", "golden", "g23_duts_data.npz")
np.savez_compressed(out, **g)
print(f"wrote {out}: {os.path.getsize(out)} bytes, PIL {PIL.__version__}; edge case seed {seed}: {d_rgb} / {d_gray} bytes differ "
      "from a single rounding")
