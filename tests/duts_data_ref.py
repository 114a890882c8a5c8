"""numpy restatement of ddm.data.DUTSDataset.__getitem__ on bytes (ddm/data.py:996-1026 of the reference): the RGB photo and its
grey map, each resized to the target with PIL's 8-bit bilinear Image.resize (sr_data_ref.resize_u8), one flip of both, ToTensor
and *2-1.  TEST INFRASTRUCTURE ONLY: the reference for fresh inputs; tests/test_duts_data_host.py pins it against PIL's own bytes
(tests/golden/g23_duts_data.npz, tools/make_golden_duts.py)."""
import numpy as np
import torch

from sr_data_ref import coeffs, hash_bytes, resize_u8, to_float  # noqa: F401  (hash_bytes / to_float: re-exported for the tests)


TARGET = (40, 56)          # non-square, no multiple of the 16x16 tile
# (photo height, width), (map height, width) of the g23 cases: up-scaling in both axes; a non-integer down-scale whose map has
# ANOTHER size than its photo; the identity in one axis; in both; up-scaling one axis and down-scaling the other; exactly 4x
CASES = [((37, 53), (37, 53)), ((97, 131), (89, 140)), ((40, 90), (40, 90)), ((40, 56), (40, 56)), ((23, 200), (23, 200)),
         ((160, 224), (160, 224))]
DRAWS = [(0, 0), (1, 1), (2, 0), (3, 0), (4, 0), (5, 1), (1, 0), (5, 0)]          # (idx, flip): indices 1 and 5 twice, both flips


def case_sources(i):
    """The sources of case i: hashed bytes, reproducible anywhere, so the golden file holds only their checksums."""
    (ph, pw), (mh, mw) = CASES[i]
    return hash_bytes((ph, pw, 3), f"duts.photo{i}"), hash_bytes((mh, mw), f"duts.map{i}")


def resize_rgb(photo, out_hw):
    """uint8 [h, w, 3] -> uint8 [H, W, 3]."""
    return resize_u8(np.ascontiguousarray(photo), tuple(out_hw), "bilinear")


def resize_gray(gmap, out_hw):
    """uint8 [h, w] -> uint8 [H, W]: a mode-L image goes through the same two passes, one byte per pixel."""
    return np.ascontiguousarray(resize_u8(np.repeat(gmap[:, :, None], 3, axis=2), tuple(out_hw), "bilinear")[:, :, 0])


def duts_pair(photo, gmap, out_hw, flip=False):
    """(rgb uint8 [H, W, 3], gray uint8 [H, W]); the flip follows the resize (data.py:982-985)."""
    rgb, gray = resize_rgb(photo, out_hw), resize_gray(gmap, out_hw)
    if flip:
        rgb, gray = rgb[:, ::-1], gray[:, ::-1]
    return np.ascontiguousarray(rgb), np.ascontiguousarray(gray)


def gray_to_float(u8):
    """uint8 [..., H, W] -> float32 [..., 1, H, W]: /255 then *2-1 (data.py:1020-1025), as torch computes it on the CPU."""
    t = torch.from_numpy(np.ascontiguousarray(u8))
    return (t.float() / 255 * 2 - 1).unsqueeze(-3).contiguous()


def resize_rounded_once(img, out_hw):
    """What a resize WITHOUT the uint8 intermediate would give: the same integer coefficients, both passes accumulated exactly
    (Python integers, 44 fractional bits), one rounding and one clip at the end.  uint8 [h, w, 3] -> uint8 [H, W, 3]."""
    H, W = out_hw
    hor = np.zeros((img.shape[0], W, 3), dtype=object)
    for i, (lo, k) in enumerate(coeffs(img.shape[1], W, "bilinear")):
        for j, kj in enumerate(k.tolist()):
            hor[:, i] += img[:, lo + j].astype(object) * kj
    out = np.zeros((H, W, 3), dtype=object)
    for i, (lo, k) in enumerate(coeffs(img.shape[0], H, "bilinear")):
        for j, kj in enumerate(k.tolist()):
            out[i] += hor[lo + j] * kj
    return np.clip((out + (1 << 43)) >> 44, 0, 255).astype(np.uint8)
