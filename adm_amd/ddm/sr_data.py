"""Super-resolution training pairs on the HIP hot path: the batches of ``ddm.data.SRDataset`` (ddm/data.py:594-658 of the reference)
made by one kernel launch from a uint8 image pool resident in device memory.

The reference makes each pair on the host with PIL: random crop of the high-resolution image [:649], ``Image.resize`` of the crop
to ``image_size // down`` with the bicubic filter [:651] (antialiased, 8 bits per channel), one horizontal-flip draw applied to
both images [:652], ``ToTensor`` and ``*2-1`` [:655-657].  PIL's resize is integer arithmetic throughout, so
``adm_sr_batch`` (adm_amd/csrc/sr_data.hip) reproduces its bytes exactly; what stays on the host is the coefficient tables
(``resample_table``: PIL's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` in Python float64, built once per shape).

``SRBatchStream`` is the batch source of train_cond_ldm.py; ``resample_image`` is the same kernel on one whole image (the
condition of ``ddm.data.SRDatasetTest``, sample_cond_ldm.py).  The draws live on the device: no ``.item()`` / ``.cpu()`` and no
dataloader workers on the per-step path.
"""
from __future__ import annotations

import math
import os
from typing import List, Sequence, Tuple

import numpy as np
import torch

from .. import hip
from ..hip import call, ptr

PRECISION_BITS = 32 - 8 - 2          # PIL: coefficients carry 22 fractional bits


def _bilinear(x: float) -> float:
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTERS = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0)}


def resample_table(in_size: int, out_size: int, filter: str = "bicubic") -> Tuple[np.ndarray, np.ndarray]:
    """(bounds int32 [out, 2] = {window start, window length}, coeffs int32 [out, ksize]) of resizing ``in_size`` samples to
    ``out_size``: PIL's coefficient computation in its operation order, in Python float64 -- support x max(scale, 1),
    center = (i + 0.5) scale, truncating int() for the window ends, clipped to the image, weights normalised by their running
    sum, int(+-0.5 + w 2^22).  ``lanczos`` raises: its weights go through sin, and bit-equality with a second libm is not promised."""
    if filter == "lanczos":
        raise NotImplementedError("inter_type 'lanczos': its weights go through sin(); only 'bicubic' and 'bilinear' are exact here")
    if filter not in _FILTERS:
        raise ValueError(f"unknown resampling filter {filter!r} (bicubic, bilinear)")
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"resample_table: sizes must be positive, got {in_size} -> {out_size}")
    fn, fsupport = _FILTERS[filter]
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeffs = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        ww, k = 0.0, []
        for x in range(xmax):
            w = fn((x + xmin - center + 0.5) * ss)
            k.append(w)
            ww += w
        for x in range(xmax):
            v = k[x] / ww if ww != 0.0 else k[x]
            coeffs[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, coeffs


def pack_bytes(images: Sequence[np.ndarray], channels: int, what: str):
    """The packing of every uint8 pool, for planes of ``channels`` bytes per pixel (3: uint8 [H,W,3], 1: uint8 [H,W]; sizes may
    differ): (bytes uint8 padded to a multiple of 4, byte offsets int64 [N], sizes int32 [N, 2])."""
    if len(images) == 0:
        raise ValueError(f"the {what} pool is empty")
    shape = "[H, W, 3]" if channels == 3 else "[H, W]"
    off, hw, total = [], [], 0
    for i, a in enumerate(images):
        if a.dtype != np.uint8 or a.ndim != (3 if channels == 3 else 2) or (channels == 3 and a.shape[2] != 3) or a.size == 0:
            raise ValueError(f"{what} {i}: expected a non-empty uint8 {shape}, got {a.dtype} {a.shape}")
        off.append(total)
        hw.append((a.shape[0], a.shape[1]))
        total += a.size
    flat = np.zeros((total + 3) // 4 * 4, dtype=np.uint8)
    for a, o in zip(images, off):
        flat[o:o + a.size] = a.reshape(-1)
    return flat, np.asarray(off, dtype=np.int64), np.asarray(hw, dtype=np.int32)


def pack_pool(images: Sequence[np.ndarray], crop_hw: Tuple[int, int]):
    """Host half of the SR pool: ``pack_bytes`` of uint8 HWC images.  An image smaller than the crop raises, as T.RandomCrop would
    (data.py:627)."""
    H, W = int(crop_hw[0]), int(crop_hw[1])
    flat, off, hw = pack_bytes(images, 3, "image")
    for i, (h, w) in enumerate(hw.tolist()):
        if h < H or w < W:
            raise ValueError(f"image {i} is {h}x{w}, smaller than the {H}x{W} crop")
    return flat, off, hw


def load_image_folder(folder: str, exts=("png", "jpg")) -> Tuple[List[np.ndarray], List[str]]:
    """Every ``*.png`` / ``*.jpg`` below ``folder`` (found recursively, extension by extension as data.py:622 lists them), decoded
    once with PIL to RGB uint8."""
    from pathlib import Path

    from PIL import Image
    paths = [p for ext in exts for p in sorted(Path(folder).rglob(f"*.{ext}"))]
    if not paths:
        raise FileNotFoundError(f"data.img_folder: no {'/'.join(exts)} image below {folder}")
    return [np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8) for p in paths], [p.name for p in paths]


class ImagePool:
    """The packed image pool and its per-image table in device memory."""

    def __init__(self, flat: torch.Tensor, off: torch.Tensor, hw: torch.Tensor):
        self.flat, self.off, self.hw = flat, off, hw
        self.n = int(off.shape[0])

    @classmethod
    def from_arrays(cls, images: Sequence[np.ndarray], crop_hw, device) -> "ImagePool":
        flat, off, hw = pack_pool(images, crop_hw)
        return cls(torch.from_numpy(flat).to(device), torch.from_numpy(off).to(device), torch.from_numpy(hw).to(device))

    @classmethod
    def from_uniform(cls, images: torch.Tensor, crop_hw) -> "ImagePool":
        """images: uint8 [N, H, W, 3] on the device (H * W * 3 need not be a multiple of 4: the tail is padded)."""
        N, H, W, C = images.shape
        if images.dtype != torch.uint8 or C != 3 or H < crop_hw[0] or W < crop_hw[1]:
            raise ValueError(f"image array must be uint8 [N, H >= {crop_hw[0]}, W >= {crop_hw[1]}, 3], got {images.dtype} {tuple(images.shape)}")
        n = N * H * W * 3
        flat = torch.zeros((n + 3) // 4 * 4, dtype=torch.uint8, device=images.device)
        flat[:n] = images.reshape(-1)
        off = torch.arange(N, device=images.device, dtype=torch.int64) * (H * W * 3)
        hw = torch.tensor([[H, W]], device=images.device, dtype=torch.int32).repeat(N, 1)
        return cls(flat, off, hw.contiguous())


class Resampler:
    """The two tables of resizing an H x W crop to h x w, in device memory."""

    def __init__(self, size, out_size, filter: str, device):
        (self.H, self.W), (self.h, self.w) = (int(size[0]), int(size[1])), (int(out_size[0]), int(out_size[1]))
        hb, hc = resample_table(self.W, self.w, filter)
        vb, vc = resample_table(self.H, self.h, filter)
        self.kh, self.kv = int(hc.shape[1]), int(vc.shape[1])
        self.hb, self.hc, self.vb, self.vc = (torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (hb, hc, vb, vc))


def _draw(v, B, device) -> torch.Tensor:
    t = torch.as_tensor(v, device=device).to(torch.int32).reshape(-1).contiguous()
    if t.numel() != B:
        raise ValueError(f"a draw has {t.numel()} entries, the batch {B}")
    return t


@torch.no_grad()
def sr_batch(pool: ImagePool, rs: Resampler, idx, top, left, flip, want_u8: bool = False):
    """One ``adm_sr_batch`` launch: (image [B,3,H,W], cond [B,3,h,w], cond_u8 [B,h,w,3] or None) for the draws idx / top / left /
    flip (int32 [B] device tensors; anything else is converted)."""
    hip.require_cuda(pool.flat, "the image pool")
    dev = pool.flat.device
    B = int(torch.as_tensor(idx).numel())
    idx, top, left, flip = (_draw(v, B, dev) for v in (idx, top, left, flip))
    image = torch.empty(B, 3, rs.H, rs.W, device=dev, dtype=torch.float32)
    cond = torch.empty(B, 3, rs.h, rs.w, device=dev, dtype=torch.float32)
    u8 = torch.empty(B, rs.h, rs.w, 3, device=dev, dtype=torch.uint8) if want_u8 else None
    call("adm_sr_batch", ptr(pool.flat), pool.flat.numel(), ptr(pool.off), ptr(pool.hw), pool.n, ptr(idx), ptr(top), ptr(left),
         ptr(flip), ptr(rs.hb), ptr(rs.hc), rs.kh, ptr(rs.vb), ptr(rs.vc), rs.kv, ptr(image), ptr(cond), ptr(u8), B, rs.H, rs.W,
         rs.h, rs.w)
    return image, cond, u8


def resample_image(img: np.ndarray, down: int, filter: str, device, want_u8: bool = False):
    """One whole uint8 [H, W, 3] image and its ``down``-times smaller copy: a pool of one image, the crop being the image, no flip."""
    H, W = img.shape[:2]
    pool = ImagePool.from_arrays([np.ascontiguousarray(img)], (H, W), device)
    rs = Resampler((H, W), (H // down, W // down), filter, device)
    z = torch.zeros(1, dtype=torch.int32, device=device)
    return sr_batch(pool, rs, z, z, z, z, want_u8)


def load_u8_array(path: str) -> np.ndarray:
    """``data.npy``: a uint8 [N,H,W,3] image array."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"data.npy: {path} does not exist")
    arr = np.load(path, allow_pickle=False)
    if arr.dtype != np.uint8 or arr.ndim != 4:
        raise ValueError(f"image array must be uint8 [N,H,W,3], got {arr.dtype} {arr.shape}")
    return arr


class PoolStream:
    """What the batch streams over an ImagePool share: the device generator, the running permutation of the image order and the
    horizontal-flip draw.  A subclass sets ``self.pool``."""

    def __init__(self, batch, device, seed, flip: bool):
        self.batch, self.device, self.flip = int(batch), device, bool(flip)
        self.gen = torch.Generator(device=device).manual_seed(seed)
        self._order = torch.empty(0, dtype=torch.int64, device=device)      # what is left of the running permutation(s)
        self._zeros = torch.zeros(self.batch, dtype=torch.int32, device=device)

    def take_indices(self) -> torch.Tensor:
        """The next ``batch`` image indices (int64): a fresh permutation per epoch, continued across the epoch boundary."""
        while self._order.numel() < self.batch:          # (sizes are host integers: no synchronisation)
            self._order = torch.cat([self._order, torch.randperm(self.pool.n, device=self.device, generator=self.gen)])
        idx, self._order = self._order[:self.batch], self._order[self.batch:]
        return idx

    def draw_flip(self) -> torch.Tensor:
        """int32 [B]: p = 0.5 with ``augment_horizontal_flip``, else zeros (no draw is consumed)."""
        if self.flip:
            return (torch.rand(self.batch, device=self.device, generator=self.gen) < 0.5).to(torch.int32)
        return self._zeros

    def __iter__(self):
        return self


class SRBatchStream(PoolStream):
    """Infinite iterator of {'image': [B,3,H,W], 'cond': [B,3,H/down,W/down]} in [-1, 1] on the GPU, keyed as ddm.data.SRDataset
    keys them (data.py:658).

    Sources, in this order: ``data.npy`` (uint8 [N,H,W,3] with H, W >= image_size); ``data.class_name: ddm.data.SRDataset`` +
    ``img_folder`` (png / jpg found recursively, decoded once with PIL at start-up into the packed ragged pool); ``data.class_name:
    synthetic`` (a pool of U(0,255) images generated on the device, so the synthetic path runs the same kernel).  Anything else
    raises.  Honours ``down`` (default 4), ``inter_type`` (default bicubic) and ``augment_horizontal_flip``.

    Draws come from the stream's device generator: the image order is a fresh permutation per epoch (DataLoader(shuffle=True),
    train_cond_ldm.py:62), top / left uniform over the valid range (T.RandomCrop), the flip with p = 0.5.  What differs from the
    reference's loader: the permutation is CONTINUED across the epoch boundary, so every batch is full; the reference's loader
    has no drop_last and can end an epoch on a short batch.  ``next_batch(idx=, top=, left=, flip=)`` accepts injected draws."""

    SYNTHETIC_IMAGES = 32

    def __init__(self, data_cfg, batch, image_size, device, seed):
        data_cfg = data_cfg or {}
        super().__init__(batch, device, seed, bool(data_cfg.get("augment_horizontal_flip", False)))          # data.py:601
        self.size = (int(image_size[0]), int(image_size[1]))
        self.down = int(data_cfg.get("down") or 4)
        self.filter = data_cfg.get("inter_type") or "bicubic"
        H, W = self.size
        if H % self.down or W % self.down:
            raise ValueError(f"image_size {self.size} is not a multiple of down = {self.down}")
        self.rs = Resampler(self.size, (H // self.down, W // self.down), self.filter, device)
        path, cls = data_cfg.get("npy"), data_cfg.get("class_name")
        if path:
            self.pool = ImagePool.from_uniform(torch.from_numpy(np.ascontiguousarray(load_u8_array(path))).to(device), self.size)
        elif cls in ("ddm.data.SRDataset", "SRDataset"):
            if not data_cfg.get("img_folder"):
                raise ValueError("data.class_name ddm.data.SRDataset needs data.img_folder")
            images, _ = load_image_folder(data_cfg.get("img_folder"))
            self.pool = ImagePool.from_arrays(images, self.size, device)
        elif cls == "synthetic":
            shape = (self.SYNTHETIC_IMAGES, H + H // 8, W + W // 8, 3)
            self.pool = ImagePool.from_uniform(torch.randint(0, 256, shape, device=device, dtype=torch.uint8, generator=self.gen),
                                               self.size)
        else:
            raise NotImplementedError(f"data.class_name {cls!r}: only ddm.data.SRDataset + img_folder, a uint8 data.npy, or "
                                      "'synthetic' (U(0,255) images, benchmarking only) are implemented")
        self._size = torch.tensor(self.size, dtype=torch.int64, device=device)

    def draw(self):
        """(idx, top, left, flip) of one batch, int32 device tensors."""
        idx = self.take_indices()
        r = torch.randint(0, 2 ** 31 - 1, (2, self.batch), device=self.device, generator=self.gen)
        span = self.pool.hw[idx].to(torch.int64) - self._size + 1          # [B, 2] valid offsets
        top, left = r[0] % span[:, 0], r[1] % span[:, 1]
        return idx.to(torch.int32), top.to(torch.int32), left.to(torch.int32), self.draw_flip()

    def next_batch(self, idx=None, top=None, left=None, flip=None, want_u8: bool = False):
        if idx is None or top is None or left is None or flip is None:
            d = self.draw()
            idx, top, left, flip = (g if v is None else v for v, g in zip((idx, top, left, flip), d))
        image, cond, u8 = sr_batch(self.pool, self.rs, idx, top, left, flip, want_u8)
        out = {"image": image, "cond": cond}
        if want_u8:
            out["cond_u8"] = u8
        return out

    def __next__(self):
        return self.next_batch()
