#!/usr/bin/env python3
"""Golden vectors for the super-resolution batches: PIL's own bytes.  Needs PIL (no GPU, no reference import: ddm.data needs
torchvision, so the steps of SRDataset.__getitem__ -- crop -> Image.resize(BICUBIC | BILINEAR) -> flip -- and of
SRDatasetTest.__getitem__ -- pad with black to multiples of 256 -> resize -- are performed here with PIL itself on recorded
inputs and draws).  Writes tests/golden/g21_sr_data.npz: input bytes, draws, output bytes, PIL's version."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sr_data_ref import hash_bytes  # noqa: E402

FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}
g = {"pil_version": np.array(PIL.__version__)}


def sr_item(img, top, left, size, down, kind, flip):
    """data.py:647-652 with the crop offset and the flip given instead of drawn."""
    H, W = size
    crop = Image.fromarray(img).convert("RGB").crop((left, top, left + W, top + H))
    mask = crop.copy().resize((W // down, H // down), resample=FILTER[kind])          # PIL sizes are (width, height)
    if flip:
        crop, mask = crop.transpose(Image.FLIP_LEFT_RIGHT), mask.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(crop), np.asarray(mask)


def resize_only(img, out_hw, kind):
    return np.asarray(Image.fromarray(img).resize((out_hw[1], out_hw[0]), resample=FILTER[kind]))


# 1: every window clipped by a border
x = hash_bytes((16, 16, 3), "sr.clipped")
g["clipped.in"] = x
g["clipped.image"], g["clipped.cond"] = sr_item(x, 0, 0, (16, 16), 4, "bicubic", False)

# 2: ragged pool, crops and flips: crop 64x48 -> 16x12
sizes = [(80, 72), (64, 48), (100, 65)]
pool = [hash_bytes((h, w, 3), f"sr.pool{i}") for i, (h, w) in enumerate(sizes)]
draws = np.array([[0, 0, 24, 1], [2, 36, 0, 0], [0, 16, 5, 1]], dtype=np.int32)          # idx, top, left, flip
for i, p in enumerate(pool):
    g[f"pool.in{i}"] = p
g["pool.draws"] = draws
pairs = [sr_item(pool[i], t, l, (64, 48), 4, "bicubic", bool(f)) for i, t, l, f in draws]
g["pool.image"] = np.stack([p[0] for p in pairs])
g["pool.cond"] = np.stack([p[1] for p in pairs])

# 3: step edges 0 / 255, another half-plane per channel: the horizontal pass over- and undershoots, so the uint8 intermediate shows
yy, xx = np.mgrid[0:32, 0:32]
x = np.stack([np.where(xx < 13, 0, 255), np.where(yy < 18, 255, 0), np.where(xx + yy < 29, 255, 0)], axis=-1).astype(np.uint8)
g["edge.in"] = x
g["edge.image"], g["edge.cond"] = sr_item(x, 0, 0, (32, 32), 4, "bicubic", False)

# 4: other tables
for tag, (H, W), (h, w), kind in (("nonint", (36, 28), (12, 9), "bicubic"), ("by8", (24, 40), (3, 5), "bicubic"),
                                 ("bilinear", (32, 48), (8, 12), "bilinear"), ("tiny", (8, 8), (2, 2), "bicubic"),
                                 ("tall", (20, 12), (5, 3), "bilinear")):
    x = hash_bytes((H, W, 3), f"sr.{tag}")
    g[f"{tag}.in"], g[f"{tag}.kind"], g[f"{tag}.cond"] = x, np.array(kind), resize_only(x, (h, w), kind)

# 5: flip before or after the resize
x = hash_bytes((64, 64, 3), "sr.fliporder")
a = resize_only(np.ascontiguousarray(x[:, ::-1]), (16, 16), "bicubic")
b = resize_only(x, (16, 16), "bicubic")[:, ::-1]
g["fliporder.equal"] = np.array(bool(np.array_equal(a, b)))

# 8: SRDatasetTest (data.py:706-715): 300x260 -> padded 512x512 -> 128x128.  Content that is constant along y in 8-row bands, so the file stays small.
yy, xx = np.mgrid[0:300, 0:260]
blocks = hash_bytes((38, 33, 2), "sr.test.blocks")          # rows repeat inside 8-row bands, which deflate finds
x = np.stack([blocks[yy // 8, xx // 8, 0], (xx * 2 + (yy // 8) * 16) % 256, blocks[yy // 8, xx // 8, 1] // 2 + xx % 8 * 16],
             axis=-1).astype(np.uint8)
img = Image.fromarray(x).convert("RGB")
w_, h_ = img.size
res = Image.new(img.mode, (-(-w_ // 256) * 256, -(-h_ // 256) * 256), (0, 0, 0))
res.paste(img, (0, 0))
mask = res.copy().resize((res.size[0] // 4, res.size[1] // 4), resample=Image.BICUBIC)
g["test.in"], g["test.cond"] = x, np.asarray(mask)

out = os.path.join(ROOT, "tests", "golden", "g21_sr_data.npz")
np.savez_compressed(out, **g)
print(f"wrote {out}: {os.path.getsize(out)} bytes, PIL {PIL.__version__}, flip order equal: {bool(g['fliporder.equal'])}")
