"""First-stage training images on the HIP hot path: the batches a KL autoencoder trains on, made by one kernel launch from ONE uint8
pool resident in device memory.

The reference's first-stage recipes read three datasets.  ``ddm.data.ImageDataset`` (ddm/data.py:140-185 of the reference) opens a
photo, ``.convert('RGB')``, resizes it to ``image_size`` with the antialiased bilinear filter [Resize -> F.resize -> Image.resize],
flips it and returns ``{'image': [3,H,W]}`` in [-1, 1].  ``ddm.data.DUTSDataset`` [:953-1026] and ``ddm.data.SketchDataset``
[:1028-1103] do the same to a pair and key the grey map, respectively the photo, as ``image`` -- the plane the recipe generates and
so the plane its first stage auto-encodes.  A first stage needs that ONE plane: ``adm_image_resize_batch``
(adm_amd/csrc/image_data.hip) is the one-plane sibling of ``adm_pair_resize_batch`` -- the same resampler (resample_u8.h), the same
table pool (``pair_data.build_table_pool``'s layout with two table ids per image), C = 3 or C = 1 bytes per pixel -- so the bytes
are PIL's, and the other plane of a pair is never decoded or held in device memory.

``ImageFolderStream``, ``DUTSMapStream`` and ``SketchPhotoStream`` are batch sources of train_vae.py (``first_stage_stream``
there); the first also serves train_uncond_dpm.py and train_uncond_ldm.py.  The draws live on the device: no ``.item()`` /
``.cpu()`` and no dataloader workers on the per-step path.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import hip
from ..hip import call, ptr
from .pair_data import (DUTS_CLASSES, SKETCH_CLASSES, check_sizes, find_duts_pairs, find_sketch_pairs, synthetic_sizes, table_pool,
                        taps)
from .sr_data import PoolStream, _draw, pack_bytes

IMAGE_CLASSES = ("ddm.data.ImageDataset", "ImageDataset")


def build_plane_tables(hw, out_hw) -> Dict[str, np.ndarray]:
    """``pair_data.table_pool`` of resizing every source size in ``hw`` ([N, 2] = (height, width)) to ``out_hw``: ``img_tab`` int32
    [N, 2] = ids of {width table, height table}."""
    H, W = int(out_hw[0]), int(out_hw[1])
    return table_pool([[(w, W), (h, H)] for h, w in np.asarray(hw).reshape(-1, 2).tolist()])


def check_plane_budget(hw, out_hw, names: Optional[Sequence[str]] = None) -> Tuple[int, int]:
    """``pair_data.check_budget``'s rule for one plane: refuse, by name, an image whose source-to-target ratio needs more LDS than a
    workgroup has; returns (max_h, max_w)."""
    label = (lambda i: f"image {i} ({names[i]})") if names else (lambda i: f"image {i}")
    return check_sizes(hw, out_hw, label, lambda i: "it is")


class PlanePool:
    """One packed pool (``channels`` = 3 or 1 bytes per pixel), its per-image tables and the table pool, in device memory."""

    def __init__(self, flat, off, hw, channels: int, out_hw, device, names=None):
        """flat: uint8 device tensor (a multiple of 4 bytes); off int64 [N] / hw int32 [N, 2]: host arrays."""
        if int(channels) not in (1, 3):
            raise ValueError(f"a plane has 1 or 3 bytes per pixel, not {channels}")
        self.channels = int(channels)
        self.out_hw = (int(out_hw[0]), int(out_hw[1]))
        self.names = list(names) if names is not None else None
        self.hw_host = np.asarray(hw, dtype=np.int32).reshape(-1, 2)
        self.n = int(self.hw_host.shape[0])
        self.max_h, self.max_w = check_plane_budget(self.hw_host, self.out_hw, self.names)
        self.kh, self.kv = taps(self.max_w, self.out_hw[1]), taps(self.max_h, self.out_hw[0])
        self.tables = build_plane_tables(self.hw_host, self.out_hw)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.flat = flat
        self.off, self.hw = dev(np.asarray(off, dtype=np.int64)), dev(self.hw_host)
        self.tab, self.tab_dir, self.img_tab = dev(self.tables["tab"]), dev(self.tables["dir"]), dev(self.tables["img_tab"])

    @classmethod
    def from_arrays(cls, images: Sequence[np.ndarray], out_hw, device, names=None) -> "PlanePool":
        """images: all uint8 [H,W,3] or all uint8 [H,W] (sizes may differ)."""
        if len(images) == 0:
            raise ValueError("the image pool is empty")
        channels = 3 if images[0].ndim == 3 else 1
        flat, off, hw = pack_bytes(images, channels, "image")
        check_plane_budget(hw, out_hw, names)          # before anything is copied to the device
        return cls(torch.from_numpy(flat).to(device), off, hw, channels, out_hw, device, names)

    @classmethod
    def from_uniform_draws(cls, sizes: Sequence[Tuple[int, int]], channels: int, out_hw, device, gen) -> "PlanePool":
        """U(0,255) bytes drawn on the device for images of the given (height, width) sizes."""
        hw = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
        check_plane_budget(hw, out_hw)
        px = hw[:, 0].astype(np.int64) * hw[:, 1] * int(channels)
        off = np.concatenate([[0], np.cumsum(px)[:-1]]).astype(np.int64)
        flat = torch.randint(0, 256, ((int(px.sum()) + 3) // 4 * 4,), device=device, dtype=torch.uint8, generator=gen)
        return cls(flat, off, hw, channels, out_hw, device)

    @property
    def nbytes(self) -> int:
        return int(self.flat.numel() + 4 * self.tab.numel())


def launch(pool: PlanePool, idx, flip, out, out_u8, B: int):
    """The raw ``adm_image_resize_batch`` call on buffers the caller owns."""
    H, W = pool.out_hw
    call("adm_image_resize_batch", ptr(pool.flat), pool.flat.numel(), ptr(pool.off), ptr(pool.hw), pool.n, pool.channels,
         ptr(pool.tab), pool.tab.numel(), ptr(pool.tab_dir), int(pool.tab_dir.shape[0]), ptr(pool.img_tab), pool.max_h, pool.max_w,
         pool.kh, pool.kv, ptr(idx), ptr(flip), ptr(out), ptr(out_u8), B, H, W)


@torch.no_grad()
def image_batch(pool: PlanePool, idx, flip, want_u8: bool = False):
    """One ``adm_image_resize_batch`` launch: (out [B,C,H,W], out_u8 [B,H,W,C] or None) for the draws idx / flip (int32 [B] device
    tensors; anything else is converted)."""
    hip.require_cuda(pool.flat, "the image pool")
    dev = pool.flat.device
    B = int(torch.as_tensor(idx).numel())
    idx, flip = _draw(idx, B, dev), _draw(flip, B, dev)
    H, W = pool.out_hw
    out = torch.empty(B, pool.channels, H, W, device=dev, dtype=torch.float32)
    out_u8 = torch.empty(B, H, W, pool.channels, device=dev, dtype=torch.uint8) if want_u8 else None
    launch(pool, idx, flip, out, out_u8, B)
    return out, out_u8


def find_images(img_folder: str, exts=("jpg", "png")):
    """The reference's discovery (data.py:161): ``*.jpg`` then ``*.png`` directly in ``img_folder`` (not below it), each sorted."""
    from pathlib import Path
    paths = [p for ext in exts for p in sorted(Path(img_folder).glob(f"*.{ext}"))]
    if not paths:
        raise FileNotFoundError(f"data.img_folder: no {'/'.join(exts)} image in {img_folder}")
    return paths


def _decode(paths, mode: str) -> List[np.ndarray]:
    """Each file decoded once with PIL and converted; an unreadable file raises and names itself."""
    from PIL import Image
    out = []
    for p in paths:
        try:
            out.append(np.asarray(Image.open(p).convert(mode), dtype=np.uint8))
        except Exception as e:
            raise OSError(f"{p} cannot be read as an image: {e}") from e
    return out


class ImageBatchStream(PoolStream):
    """Infinite iterator of {'image': [B,C,H,W]} in [-1, 1] on the GPU from a ``PlanePool``: what the three first-stage sources
    share.  A subclass names its dataset (``CLASSES``, ``LABEL``), its channel count and its config key, and lists its files
    (``paths``).

    The image order is ``PoolStream``'s (a fresh permutation per epoch, continued across the boundary, so every batch is full); the
    flip is drawn with p = 0.5 when ``augment_horizontal_flip`` (default: the class's own).  ``class_name: synthetic`` with
    ``synthetic_of`` naming the class builds a pool of U(0,255) bytes at ``synthetic_sizes`` ([(h, w)], default a few sizes around
    ``image_size``), so the synthetic path runs the same kernel.  ``next_batch(idx=, flip=)`` accepts injected draws."""

    SYNTHETIC_IMAGES = 32
    CLASSES: Tuple[str, ...] = ()
    LABEL = ""
    CHANNELS = 3
    MODE = "RGB"
    ROOT_KEY = "img_folder"
    FLIP_DEFAULT = False

    @staticmethod
    def paths(cfg):
        raise NotImplementedError

    def __init__(self, data_cfg, batch, image_size, device, seed):
        data_cfg = data_cfg or {}
        full = self.CLASSES[0]
        super().__init__(batch, device, seed, bool(data_cfg.get("augment_horizontal_flip", self.FLIP_DEFAULT)))
        self.size = (int(image_size[0]), int(image_size[1]))
        self.channels = self.CHANNELS
        cls = data_cfg.get("class_name")
        if cls in self.CLASSES:
            if not data_cfg.get(self.ROOT_KEY):
                raise ValueError(f"data.class_name {full} needs data.{self.ROOT_KEY}")
            files = self.paths(data_cfg)
            self.pool = PlanePool.from_arrays(_decode(files, self.MODE), self.size, device, [p.name for p in files])
        elif cls == "synthetic" and data_cfg.get("synthetic_of") in self.CLASSES:
            sizes = data_cfg.get("synthetic_sizes") or synthetic_sizes(self.size, self.SYNTHETIC_IMAGES)
            self.pool = PlanePool.from_uniform_draws([tuple(s) for s in sizes], self.CHANNELS, self.size, device, self.gen)
        else:
            raise NotImplementedError(f"data.class_name {cls!r}: only {full} + {self.ROOT_KEY}, or 'synthetic' with "
                                      f"synthetic_of: {full} (U(0,255) images, benchmarking only) are implemented")
        print(f"{self.LABEL} pool: {self.pool.n} images of {self.channels} channel(s), {len(self.pool.tables['keys'])} resize tables, "
              f"{self.pool.nbytes / 2 ** 20:.1f} MiB resident in device memory")

    def draw(self):
        """(idx, flip) of one batch, int32 device tensors."""
        return self.take_indices().to(torch.int32), self.draw_flip()

    def next_batch(self, idx=None, flip=None, want_u8: bool = False):
        if idx is None or flip is None:
            d = self.draw()
            idx, flip = (g if v is None else v for v, g in zip((idx, flip), d))
        image, u8 = image_batch(self.pool, idx, flip, want_u8)
        out = {"image": image}
        if want_u8:
            out["image_u8"] = u8
        return out

    def __next__(self):
        return self.next_batch()


class ImageFolderStream(ImageBatchStream):
    """``ddm.data.ImageDataset`` + ``img_folder`` (the CelebA-HQ first stage and latent recipes): every ``*.jpg`` then ``*.png`` in
    the folder itself, ``.convert('RGB')``; ``augment_horizontal_flip`` defaults to False as in the class (data.py:148)."""

    CLASSES = IMAGE_CLASSES
    LABEL = "image"
    paths = staticmethod(lambda cfg: find_images(cfg.get("img_folder")))


class DUTSMapStream(ImageBatchStream):
    """``ddm.data.DUTSDataset`` + ``data_root``: the ground-truth MAPS only (``find_duts_pairs``, ``.convert('L')``), one channel --
    the ``image`` of the saliency recipe, which its first stage auto-encodes.  The photos are found (a map is located through its
    photo) but never opened."""

    CLASSES = DUTS_CLASSES
    LABEL = "DUTS map"
    CHANNELS, MODE, ROOT_KEY = 1, "L", "data_root"
    paths = staticmethod(lambda cfg: [m for _, m in find_duts_pairs(cfg.get("data_root"), cfg.get("split") or "train")])


class SketchPhotoStream(ImageBatchStream):
    """``ddm.data.SketchDataset`` + ``data_root``: the PHOTOS only (``find_sketch_pairs``, ``.convert('RGB')``) -- the ``image`` of
    the sketch-to-image recipe.  The sketches are located, never opened."""

    CLASSES = SKETCH_CLASSES
    LABEL = "sketch photo"
    ROOT_KEY = "data_root"
    paths = staticmethod(lambda cfg: [p for p, _ in find_sketch_pairs(cfg.get("data_root"), cfg.get("split") or "train")])


def stream_class(data_cfg):
    """The stream of this module that serves ``data_cfg`` (its ``class_name``, or its ``synthetic_of`` under ``class_name:
    synthetic``), or None: the ``first_stage`` column of ``datasets.DATASETS``, where it is one of the one-plane streams."""
    from .datasets import DATASETS, dataset_of          # (the table imports this module's classes)
    key = dataset_of(data_cfg)
    picked = DATASETS[key].first_stage if key else None
    return picked if picked is not None and issubclass(picked, ImageBatchStream) else None
