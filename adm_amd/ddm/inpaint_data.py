"""In-painting training triples on the HIP hot path: the batches of ``ddm.data.InpaintDataset`` (ddm/data.py:339-476 of the
reference) made from the uint8 image pool of ``sr_data.ImagePool`` with no host round trip per step.

The reference makes each item on the host: numpy draws -> rectangles filled into a numpy mask and free-form strokes drawn with
PIL's ``ImageDraw`` (``RandomBrush``) -> redrawn while the hole ratio is 0 or 1 -> two flips of the mask -> ``mask * image``.
Here the draws are ``torch.rand`` / ``torch.randn`` device tensors in a FIXED slot table (include/adm_hip.h, mirrored
below), ``adm_inpaint_masks`` turns them into primitive lists in fp64 and decides the rejection loop analytically over
``CANDIDATES`` candidates per sample, and ``adm_inpaint_batch`` rasterises the lists in integer arithmetic and writes
{'image', 'cond', 'ori_mask'} in one launch.  tests/inpaint_ref.py restates both kernels in NumPy, bit for bit.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import hip
from ..hip import call, ptr
from .sr_data import ImagePool, PoolStream, load_u8_array

# The slot table of include/adm_hip.h (ADM_INP_*); tests/test_inpaint_host.py holds the two together.
CANDIDATES = 4
RECTS, STROKES, VERTS, SEGMENTS = 4, 7, 18, 17
U_NRECT_SMALL, U_RECT, U_NRECT_BIG, U_NSTROKE, U_STROKE, STROKE_U, U_FLIP, NU, NZ = 0, 1, 17, 18, 19, 25, 194, 196, 119
# inside a stroke's STROKE_U slots
S_NUM_VERTEX, S_ANGLE_MIN, S_ANGLE_MAX, S_ANGLES, S_START, S_WIDTH, S_DISCARD = 0, 1, 2, 3, 20, 22, 23

PRIM_KEYS = ("rects", "verts", "nverts", "widths", "flips")
HOLDOUT = 2000          # data.py:360-363: the last 2000 sorted files are the test split


def check_hole_range(hole_range):
    if hole_range is not None and [float(v) for v in hole_range] != [0.0, 1.0]:
        raise NotImplementedError(f"data.hole_range {list(hole_range)}: only [0, 1] (what every config uses) is built; another range "
                                  "makes the rejection loop depend on the rasterised hole ratio")


@torch.no_grad()
def inpaint_masks(u: torch.Tensor, z: torch.Tensor, size: int, fallback: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """One ``adm_inpaint_masks`` launch: draws u float32 [B, CANDIDATES, NU] in [0, 1) and z float32 [B, CANDIDATES, NZ] ~ N(0, 1) ->
    {'rects' [B,4,4], 'verts' [B,7,18,2], 'nverts' [B,7], 'widths' [B,7], 'flips' [B,2], 'chosen' [B]} (int32).  ``fallback`` (int32
    [1], device) is incremented once per sample whose candidates were all empty."""
    hip.require_cuda(u, "the uniform draws")
    hip.require_cuda(z, "the normal draws")
    B = int(u.shape[0])
    if tuple(u.shape) != (B, CANDIDATES, NU) or tuple(z.shape) != (B, CANDIDATES, NZ):
        raise ValueError(f"draws must be [B, {CANDIDATES}, {NU}] and [B, {CANDIDATES}, {NZ}], got {tuple(u.shape)} and {tuple(z.shape)}")
    u, z = u.to(torch.float32).contiguous(), z.to(torch.float32).contiguous()
    dev = u.device
    if fallback is None:
        fallback = torch.zeros(1, dtype=torch.int32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    p = {"rects": torch.empty(B, RECTS, 4, **i32), "verts": torch.empty(B, STROKES, VERTS, 2, **i32),
         "nverts": torch.empty(B, STROKES, **i32), "widths": torch.empty(B, STROKES, **i32), "flips": torch.empty(B, 2, **i32),
         "chosen": torch.empty(B, **i32)}
    call("adm_inpaint_masks", ptr(u), ptr(z), ptr(p["rects"]), ptr(p["verts"]), ptr(p["nverts"]), ptr(p["widths"]), ptr(p["flips"]),
         ptr(p["chosen"]), ptr(fallback), B, int(size))
    return p


def _prim(prims, key, shape, dev) -> torch.Tensor:
    t = torch.as_tensor(prims[key], device=dev).to(torch.int32).contiguous()
    if tuple(t.shape) != shape:
        raise ValueError(f"prims[{key!r}] must be {shape}, got {tuple(t.shape)}")
    return t


@torch.no_grad()
def inpaint_batch(pool: ImagePool, idx, flip, prims, size: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One ``adm_inpaint_batch`` launch: (image [B,3,S,S], cond [B,3,S,S], ori_mask [B,1,S,S]) for image indices ``idx`` and image flips
    ``flip`` (int32 [B]) and the primitive lists ``prims`` (what ``inpaint_masks`` returns; anything else is converted)."""
    hip.require_cuda(pool.flat, "the image pool")
    dev, S = pool.flat.device, int(size)
    idx = torch.as_tensor(idx, device=dev).to(torch.int32).reshape(-1).contiguous()
    B = int(idx.numel())
    flip = torch.as_tensor(flip, device=dev).to(torch.int32).reshape(-1).contiguous()
    if flip.numel() != B:
        raise ValueError(f"a draw has {flip.numel()} entries, the batch {B}")
    shapes = {"rects": (B, RECTS, 4), "verts": (B, STROKES, VERTS, 2), "nverts": (B, STROKES), "widths": (B, STROKES), "flips": (B, 2)}
    r, v, nv, w, mf = (_prim(prims, k, shapes[k], dev) for k in PRIM_KEYS)
    image = torch.empty(B, 3, S, S, device=dev, dtype=torch.float32)
    cond = torch.empty(B, 3, S, S, device=dev, dtype=torch.float32)
    mask = torch.empty(B, 1, S, S, device=dev, dtype=torch.float32)
    call("adm_inpaint_batch", ptr(pool.flat), pool.flat.numel(), ptr(pool.off), ptr(pool.hw), pool.n, ptr(idx), ptr(flip), ptr(r),
         ptr(v), ptr(nv), ptr(w), ptr(mf), ptr(image), ptr(cond), ptr(mask), B, S)
    return image, cond, mask


@torch.no_grad()
def inpaint_compose(mask: torch.Tensor, cond: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """mask * (cond + 1) / 2 + (1 - mask) * x (ddm_const_2.py:629): mask [B,1,H,W], cond / x [B,C,H,W] float32."""
    hip.require_cuda(x, "the sample")
    B, C, H, W = x.shape
    if tuple(mask.shape) != (B, 1, H, W) or tuple(cond.shape) != (B, C, H, W):
        raise ValueError(f"compose: mask {tuple(mask.shape)} / cond {tuple(cond.shape)} do not fit the sample {tuple(x.shape)}")
    mask, cond, x = (t.to(device=x.device, dtype=torch.float32).contiguous() for t in (mask, cond, x))
    out = torch.empty_like(x)
    call("adm_inpaint_compose", ptr(mask), ptr(cond), ptr(x), ptr(out), B, C, H * W)
    return out


def load_inpaint_folder(folder: str, split: str = "train") -> Tuple[List[np.ndarray], List[str]]:
    """``*.jpg`` directly in ``folder`` (not recursive), sorted; ``train`` drops the last 2000, ``test`` keeps them (data.py:359-363)."""
    from pathlib import Path

    from PIL import Image
    if split not in ("train", "test"):
        raise ValueError(f"data.split must be 'train' or 'test', got {split!r}")
    paths = sorted(Path(folder).glob("*.jpg"))
    n_all = len(paths)
    paths = paths[:-HOLDOUT] if split == "train" else paths[-HOLDOUT:]
    if not paths:
        raise ValueError(f"data.img_folder {folder}: {n_all} jpg files, so split {split!r} is empty (the last {HOLDOUT} sorted files "
                         "are the test split, the rest the train split)")
    return [np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8) for p in paths], [p.name for p in paths]


def check_square(images, size):
    """The reference sizes the mask by the image's height and never resizes (data.py:391-395), so an image must be square and equal
    to image_size for mask, image and model to fit."""
    S = int(size[0])
    if int(size[1]) != S:
        raise ValueError(f"in-painting needs a square image_size, got {tuple(size)}")
    for i, a in enumerate(images):
        if a.shape[0] != S or a.shape[1] != S:
            raise ValueError(f"image {i} is {a.shape[0]}x{a.shape[1]}: in-painting images must be square and equal to image_size {S}")
    return S


class InpaintBatchStream(PoolStream):
    """Infinite iterator of {'image': [B,3,S,S], 'cond': [B,3,S,S], 'ori_mask': [B,1,S,S]} on the GPU, keyed as
    ddm.data.InpaintDataset keys them (data.py:403; 'img_name' is left out: nothing in training reads it).

    Sources, in this order: ``data.npy`` (uint8 [N,S,S,3]); ``data.class_name: ddm.data.InpaintDataset`` + ``img_folder`` (``*.jpg``, not
    recursive, sorted, split by ``data.split``); ``data.class_name: synthetic`` (U(0,255) images made on the device; train_cond_ldm.py
    reads ``data.synthetic_of`` to tell whose batches a synthetic pool stands for).  Image order and
    ``augment_horizontal_flip`` behave as in SRBatchStream (the flip mirrors the image only, never the mask: data.py:372, 395-399).
    ``fallbacks`` (int32 [1] on the device) counts samples whose CANDIDATES candidates were all empty: their mask is all ones."""

    SYNTHETIC_IMAGES = 32

    def __init__(self, data_cfg, batch, image_size, device, seed):
        data_cfg = data_cfg or {}
        super().__init__(batch, device, seed, bool(data_cfg.get("augment_horizontal_flip", False)))
        check_hole_range(data_cfg.get("hole_range"))
        size = (int(image_size[0]), int(image_size[1]))
        self.size = check_square([], size)
        S = self.size
        path, cls = data_cfg.get("npy"), data_cfg.get("class_name")
        self.names = None          # file names of the pool's images, when they came from a folder
        if path:
            arr = load_u8_array(path)
            check_square(arr[:1], size)
            self.pool = ImagePool.from_uniform(torch.from_numpy(np.ascontiguousarray(arr)).to(device), size)
        elif cls in ("ddm.data.InpaintDataset", "InpaintDataset"):
            if not data_cfg.get("img_folder"):
                raise ValueError("data.class_name ddm.data.InpaintDataset needs data.img_folder")
            images, self.names = load_inpaint_folder(data_cfg.get("img_folder"), data_cfg.get("split") or "train")
            check_square(images, size)
            self.pool = ImagePool.from_arrays(images, size, device)
        elif cls == "synthetic":
            self.pool = ImagePool.from_uniform(torch.randint(0, 256, (self.SYNTHETIC_IMAGES, S, S, 3), device=device, dtype=torch.uint8,
                                                             generator=self.gen), size)
        else:
            raise NotImplementedError(f"data.class_name {cls!r}: only ddm.data.InpaintDataset + img_folder, a uint8 data.npy, or "
                                      "'synthetic' (U(0,255) images, benchmarking only) are implemented")
        self.fallbacks = torch.zeros(1, dtype=torch.int32, device=device)

    def draw(self):
        """(idx int32 [B], flip int32 [B], u float32 [B, CANDIDATES, NU], z float32 [B, CANDIDATES, NZ]) of one batch."""
        idx = self.take_indices()
        flip = self.draw_flip()
        u = torch.rand(self.batch, CANDIDATES, NU, device=self.device, generator=self.gen)
        z = torch.randn(self.batch, CANDIDATES, NZ, device=self.device, generator=self.gen)
        return idx.to(torch.int32), flip, u, z

    def next_batch(self, idx=None, flip=None, u=None, z=None, prims=None):
        """Every draw is injectable; ``prims`` (primitive lists) replaces u / z altogether."""
        if idx is None or flip is None or (prims is None and (u is None or z is None)):
            d = self.draw()
            idx, flip, u, z = (g if v is None else v for v, g in zip((idx, flip, u, z), d))
        if prims is None:
            prims = inpaint_masks(torch.as_tensor(u, device=self.device), torch.as_tensor(z, device=self.device), self.size,
                                  self.fallbacks)
        image, cond, mask = inpaint_batch(self.pool, idx, flip, prims, self.size)
        return {"image": image, "cond": cond, "ori_mask": mask}

    def __next__(self):
        return self.next_batch()
