"""Depth-estimation pairs on the HIP hot path: the batches of ``ddm.data.NYUDv2DepthDataset`` (ddm/data.py:834-887 of the reference)
made by one kernel launch from a uint8 photo pool and a 16-BIT depth pool resident in device memory.

The reference makes each item on the host with PIL: ``rgb_*.jpg`` and its ``sync_depth_*.png`` (16 bits, millimetres) are cropped to
the fixed box (41, 45, 601, 471) [:875-876] -- 426 rows x 560 columns, the Eigen evaluation crop -- and, for ``split: train``, to one
``RandomCrop(image_size)`` with one flip draw for both [:877-878]; the photo becomes ``to_tensor * 2 - 1``, the depth
``float32(depth) / 10000 * 2 - 1`` without clipping [:879-886]; the keys are ``{'image': depth [1,H,W], 'cond': photo [3,H,W]}``.
Nothing is resized, so ``adm_depth_batch`` (adm_amd/csrc/depth_data.hip) is addressing and two float32 operations per value, equal
bit for bit to NumPy's.

What differs from the reference (README, "Depth estimation"): every split other than ``test`` gets the train transform (the
reference's ``split: full`` would feed whole 426x560 frames to an autoencoder that decodes 424 rows); a frame smaller than the box and
a missing depth file are refused by name when the pool is built (PIL would pad with black, the loader would raise mid-epoch).

``DepthBatchStream`` is a batch source of train_cond_ldm.py and, with ``split: test``, of sample_cond_ldm.py (whole boxed frames, in
order); ``DepthMapStream`` -- the depth plane only, one channel -- of train_vae.py.  The draws live on the device: no ``.item()`` /
``.cpu()`` and no dataloader workers on the per-step path.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import hip
from ..hip import call, ptr
from .sr_data import PoolStream, _draw, pack_bytes

DEPTH_CLASSES = ("ddm.data.NYUDv2DepthDataset", "NYUDv2DepthDataset")
BORDER_CROP = (41, 45, 601, 471)          # PIL's (left, upper, right, lower), data.py:875-876
DEPTH_UNITS = 10000                       # raw units per depth fraction 1.0: 10 m in millimetres (data.py:882)


def check_box(box) -> Tuple[int, int, int, int]:
    """``data.border_crop`` as four integers (left, upper, right, lower) with a positive area and no negative corner."""
    try:
        left, upper, right, lower = (int(v) for v in box)
    except (TypeError, ValueError):
        raise ValueError(f"data.border_crop must be four integers (left, upper, right, lower), got {box!r}") from None
    if left < 0 or upper < 0 or right <= left or lower <= upper:
        raise ValueError(f"data.border_crop {(left, upper, right, lower)}: (left, upper, right, lower) must be non-negative with "
                         "right > left and lower > upper")
    return left, upper, right, lower


def check_frames(rgb_hw, depth_hw, box, names: Optional[Sequence[str]] = None):
    """The two rules every depth pool is built under, each refusal naming the pair: the planes of a pair agree in size, and a frame
    holds the whole box (PIL would pad a smaller one with black).  Either table may be None (a pool of one plane)."""
    left, upper, right, lower = check_box(box)
    label = (lambda i: f"pair {i} ({names[i]})") if names is not None else (lambda i: f"pair {i}")
    tabs = [np.asarray(t).reshape(-1, 2) for t in (rgb_hw, depth_hw) if t is not None]
    if len(tabs) == 2:
        if tabs[0].shape != tabs[1].shape:
            raise ValueError(f"{tabs[0].shape[0]} photos but {tabs[1].shape[0]} depth maps")
        for i, (r, d) in enumerate(zip(tabs[0].tolist(), tabs[1].tolist())):
            if r != d:
                raise ValueError(f"{label(i)}: its photo is {r[0]}x{r[1]} but its depth map is {d[0]}x{d[1]}")
    for i, (h, w) in enumerate(tabs[0].tolist()):
        if h < lower or w < right:
            raise ValueError(f"{label(i)}: the frame is {h}x{w}, smaller than the border box {(left, upper, right, lower)} "
                             f"(which needs {lower} rows and {right} columns)")


def pack_depth(maps: Sequence[np.ndarray]):
    """The 16-bit pool: uint16 [H, W] planes (sizes may differ) as little-endian bytes -- (bytes uint8 padded to a multiple of 4, byte
    offsets int64 [N], all even, sizes int32 [N, 2])."""
    if len(maps) == 0:
        raise ValueError("the depth pool is empty")
    for i, a in enumerate(maps):
        if a.dtype != np.uint16 or a.ndim != 2 or a.size == 0:
            raise ValueError(f"depth map {i}: expected a non-empty uint16 [H, W], got {a.dtype} {a.shape}")
    px = np.asarray([a.size for a in maps], dtype=np.int64)
    off = 2 * np.concatenate([[0], np.cumsum(px)[:-1]]).astype(np.int64)
    flat = np.zeros((2 * int(px.sum()) + 3) // 4 * 4, dtype=np.uint8)
    for a, o in zip(maps, off.tolist()):
        flat[o:o + 2 * a.size] = np.ascontiguousarray(a).astype("<u2").reshape(-1).view(np.uint8)
    return flat, off, np.asarray([a.shape for a in maps], dtype=np.int32)


class DepthPool:
    """The photo pool (3 bytes per pixel; None for a pool of depth maps only), the 16-bit depth pool, their per-image tables and the
    border box, in device memory."""

    def __init__(self, rgb_flat, rgb_off, rgb_hw, depth_flat, depth_off, depth_hw, box, device, names=None):
        """*_flat: uint8 device tensors (a multiple of 4 bytes); *_off int64 [N] / *_hw int32 [N, 2]: host arrays."""
        self.box = check_box(box)
        self.names = list(names) if names is not None else None
        check_frames(rgb_hw if rgb_flat is not None else None, depth_hw, self.box, self.names)
        depth_off = np.asarray(depth_off, dtype=np.int64)
        if (depth_off & 1).any():
            raise ValueError("a depth image starts at an odd byte: the pool is read in 16-bit units")
        self.hw_host = np.asarray(depth_hw, dtype=np.int32).reshape(-1, 2)
        self.n = int(self.hw_host.shape[0])
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.rgb, self.depth = rgb_flat, depth_flat
        self.depth_off, self.depth_hw = dev(depth_off), dev(self.hw_host)
        self.rgb_off = dev(np.asarray(rgb_off, dtype=np.int64)) if rgb_flat is not None else None
        self.rgb_hw = dev(np.asarray(rgb_hw, dtype=np.int32).reshape(-1, 2)) if rgb_flat is not None else None

    @property
    def frame(self) -> Tuple[int, int]:
        """(rows, columns) the box leaves of every frame."""
        left, upper, right, lower = self.box
        return lower - upper, right - left

    @classmethod
    def from_arrays(cls, photos: Optional[Sequence[np.ndarray]], depths: Sequence[np.ndarray], box, device, names=None) -> "DepthPool":
        """photos: uint8 [H,W,3] or None; depths: uint16 [H,W] (sizes may differ from pair to pair, not within one)."""
        df, do, dh = pack_depth(depths)
        rf = ro = rh = None
        if photos is not None:
            rf, ro, rh = pack_bytes(photos, 3, "photo")
        check_frames(rh, dh, box, names)          # before anything is copied to the device
        return cls(None if rf is None else torch.from_numpy(rf).to(device), ro, rh, torch.from_numpy(df).to(device), do, dh, box,
                   device, names)

    @classmethod
    def from_uniform_draws(cls, sizes: Sequence[Tuple[int, int]], box, device, gen, photos: bool = True) -> "DepthPool":
        """U(0,255) photo bytes and U(0,10000) depths drawn on the device for pairs of the given (height, width) sizes."""
        hw = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
        check_frames(hw if photos else None, hw, box)
        px = hw[:, 0].astype(np.int64) * hw[:, 1]
        off = np.concatenate([[0], np.cumsum(px)[:-1]]).astype(np.int64)
        total = int(px.sum())
        d16 = torch.randint(0, DEPTH_UNITS + 1, ((total + 1) // 2 * 2,), device=device, dtype=torch.int16, generator=gen)
        rgb = None
        if photos:
            rgb = torch.randint(0, 256, ((3 * total + 3) // 4 * 4,), device=device, dtype=torch.uint8, generator=gen)
        return cls(rgb, 3 * off, hw, d16.view(torch.uint8), 2 * off, hw, box, device)

    @property
    def nbytes(self) -> int:
        return int(self.depth.numel() + (self.rgb.numel() if self.rgb is not None else 0))


def launch(pool: DepthPool, idx, top, left, flip, image, cond, B: int, H: int, W: int):
    """The raw ``adm_depth_batch`` call on buffers the caller owns (``image`` or ``cond`` may be None)."""
    if cond is not None and pool.rgb is None:
        raise ValueError("this pool holds no photos: it makes the depth plane only")
    rgb = pool.rgb if cond is not None else None
    call("adm_depth_batch", ptr(rgb), 0 if rgb is None else rgb.numel(), ptr(pool.rgb_off if rgb is not None else None),
         ptr(pool.rgb_hw if rgb is not None else None), ptr(pool.depth), pool.depth.numel(), ptr(pool.depth_off), ptr(pool.depth_hw),
         pool.n, *pool.box, ptr(idx), ptr(top), ptr(left), ptr(flip), ptr(image), ptr(cond), B, H, W)


@torch.no_grad()
def depth_batch(pool: DepthPool, idx, top, left, flip, size, image: bool = True, cond: bool = True):
    """One ``adm_depth_batch`` launch: (image [B,1,H,W] or None, cond [B,3,H,W] or None) for the draws idx / top / left / flip (int32
    [B] device tensors; anything else is converted).  A crop larger than the boxed frame raises, as T.RandomCrop would."""
    hip.require_cuda(pool.depth, "the depth pool")
    dev = pool.depth.device
    H, W = int(size[0]), int(size[1])
    fh, fw = pool.frame
    if H > fh or W > fw or H <= 0 or W <= 0:
        raise ValueError(f"a {H}x{W} crop does not fit the {fh}x{fw} frame the border box {pool.box} leaves")
    B = int(torch.as_tensor(idx).numel())
    idx, top, left, flip = (_draw(v, B, dev) for v in (idx, top, left, flip))
    img = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32) if image else None
    cnd = torch.empty(B, 3, H, W, device=dev, dtype=torch.float32) if cond else None
    launch(pool, idx, top, left, flip, img, cnd, B, H, W)
    return img, cnd


def find_nyud_pairs(data_root: str, split: str = "train"):
    """[(photo path, depth path)] sorted by photo path: the reference's discovery (data.py:845-858) -- every ``*.jpg`` below
    ``data_root/<split>`` for ``train`` / ``test`` (any other split: ``data_root`` itself), its depth file in the same folder under the
    name with ``rgb_`` -> ``sync_depth_`` and ``.jpg`` -> ``.png``.  DEVIATION: a missing depth file raises here and names itself; the
    reference's loader would raise in a worker, mid-epoch."""
    from pathlib import Path
    folder = Path(data_root) / split if split in ("train", "test") else Path(data_root)
    photos = sorted(folder.rglob("*.jpg"))
    if not photos:
        raise FileNotFoundError(f"data.data_root: no jpg photo below {folder}")
    pairs = []
    for p in photos:
        d = p.parent / p.name.replace("rgb_", "sync_depth_").replace(".jpg", ".png")
        if not d.is_file():
            raise FileNotFoundError(f"the depth map of {p} is missing: {d}")
        pairs.append((p, d))
    return pairs


def read_depth_png(path) -> np.ndarray:
    """A depth png as uint16 [H, W] (Pillow opens the 16-bit file as mode ``I;16``; an 8-bit or 32-bit integer file whose values fit is
    taken too).  Anything else raises and names the file."""
    from PIL import Image
    try:
        arr = np.array(Image.open(path))
    except Exception as e:
        raise OSError(f"{path} cannot be read as an image: {e}") from e
    if arr.ndim != 2 or arr.dtype.kind not in "ui" or arr.size == 0 or int(arr.min()) < 0 or int(arr.max()) > 65535:
        raise ValueError(f"{path}: expected a one-channel integer depth image within 16 bits, got {arr.dtype} {arr.shape}")
    return arr.astype(np.uint16)


def write_depth_png(path, units: np.ndarray):
    """uint16 [H, W] raw depth units as a 16-bit png (mode ``I;16``)."""
    from PIL import Image
    units = np.ascontiguousarray(units)
    if units.dtype != np.uint16 or units.ndim != 2:
        raise ValueError(f"expected uint16 [H, W], got {units.dtype} {units.shape}")
    Image.fromarray(units).save(path)


def load_nyud(data_root: str, split: str = "train", box=BORDER_CROP, photos: bool = True):
    """(photos uint8 [h,w,3] or None, depths uint16 [h,w], photo file names): decoded once, ``.convert('RGB')`` for the photo and the
    16-bit plane as it is (data.py:873-874); only the boxed region of each plane is kept, so the arrays are all lower-upper x
    right-left.  A frame smaller than the box, a pair of two sizes and an unreadable file raise and name the file.  With
    ``photos=False`` the photos are located (a depth file is found through its photo) but never opened."""
    from PIL import Image
    left, upper, right, lower = check_box(box)
    pairs = find_nyud_pairs(data_root, split)
    rgbs, depths, names = ([] if photos else None), [], []
    for p, d in pairs:
        depth = read_depth_png(d)
        check_frames(None, [depth.shape], box, [p.name])
        if photos:
            try:
                rgb = np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8)
            except Exception as e:
                raise OSError(f"{p} cannot be read as an image: {e}") from e
            check_frames([rgb.shape[:2]], [depth.shape], box, [p.name])
            rgbs.append(np.ascontiguousarray(rgb[upper:lower, left:right]))
        depths.append(np.ascontiguousarray(depth[upper:lower, left:right]))
        names.append(p.name)
    return rgbs, depths, names


def synthetic_sizes(box, n: int) -> List[Tuple[int, int]]:
    """A few frame sizes that hold ``box``: the box's own lower-right corner exactly, and two larger frames (for the default box the
    second is NYUv2's 480x640)."""
    _, _, right, lower = check_box(box)
    kinds = [(lower, right), (lower + 9, right + 39), (lower + 24, right + 16)]
    return [kinds[i % len(kinds)] for i in range(n)]


class DepthBatchStream(PoolStream):
    """Infinite iterator of {'image': depth [B,1,H,W], 'cond': photo [B,3,H,W]} on the GPU, keyed in the order
    ddm.data.NYUDv2DepthDataset keys them (data.py:887); the photo in [-1, 1], the depth ``raw / 10000 * 2 - 1``, unclipped.

    Sources, in this order: ``data.class_name: ddm.data.NYUDv2DepthDataset`` + ``data_root`` (``load_nyud``: decoded once at start-up,
    the boxed region kept); ``data.class_name: synthetic`` with ``synthetic_of: ddm.data.NYUDv2DepthDataset`` (a few frame sizes of
    U(0,255) bytes and U(0,10000) depths drawn on the device, through the same kernel).  Anything else raises.  Honours
    ``augment_horizontal_flip`` and ``border_crop`` (default [41, 45, 601, 471]; PIL's left, upper, right, lower).

    Every split but ``test`` draws as SRBatchStream does: the image order a fresh permutation per epoch continued across the boundary
    (every batch is full), top / left uniform over the valid offsets inside the boxed frame, the flip with p = 0.5, one draw for both
    planes.  ``split: test`` walks the pairs in sorted order and yields WHOLE boxed frames, unflipped, with ``img_name`` (the photo's)
    and ``ori_size``; ``image_size`` is not read.  An ``image_size`` larger than the boxed frame raises, as T.RandomCrop would.
    ``next_batch(idx=, top=, left=, flip=)`` accepts injected draws."""

    SYNTHETIC_PAIRS = 12
    PHOTOS = True
    LABEL = "depth"
    SYNTHETIC_NAME = "rgb_{:05d}.jpg"

    def __init__(self, data_cfg, batch, image_size, device, seed):
        data_cfg = data_cfg or {}
        full = DEPTH_CLASSES[0]
        self.split = data_cfg.get("split") or "train"
        self.test = self.split == "test"
        super().__init__(batch, device, seed, not self.test and bool(data_cfg.get("augment_horizontal_flip", False)))
        self.box = check_box(data_cfg.get("border_crop") or BORDER_CROP)
        fh, fw = self.box[3] - self.box[1], self.box[2] - self.box[0]
        self.size = (fh, fw) if self.test else (int(image_size[0]), int(image_size[1]))
        if self.size[0] > fh or self.size[1] > fw:
            raise ValueError(f"image_size {self.size[0]}x{self.size[1]} is larger than the {fh}x{fw} frame data.border_crop "
                             f"{list(self.box)} leaves: T.RandomCrop raises for a crop larger than its image")
        cls = data_cfg.get("class_name")
        if cls in DEPTH_CLASSES:
            if not data_cfg.get("data_root"):
                raise ValueError(f"data.class_name {full} needs data.data_root")
            photos, depths, names = load_nyud(data_cfg.get("data_root"), self.split, self.box, self.PHOTOS)
            self.pool = DepthPool.from_arrays(photos, depths, (0, 0, fw, fh), device, names)          # (only the box is resident)
        elif cls == "synthetic" and data_cfg.get("synthetic_of") in DEPTH_CLASSES:
            self.pool = DepthPool.from_uniform_draws(synthetic_sizes(self.box, self.SYNTHETIC_PAIRS), self.box, device, self.gen,
                                                     self.PHOTOS)
        else:
            raise NotImplementedError(f"data.class_name {cls!r}: only {full} + data_root, or 'synthetic' with "
                                      f"synthetic_of: {full} (U(0,255) photos and U(0,10000) depths, benchmarking only) are implemented")
        self.names = self.pool.names or [self.SYNTHETIC_NAME.format(i) for i in range(self.pool.n)]
        self.ori_sizes = [(fh, fw)] * self.pool.n
        self._span = (fh - self.size[0] + 1, fw - self.size[1] + 1)          # valid offsets: every boxed frame has one size
        self._cursor = 0          # split: test
        planes = "photo + depth planes" if self.PHOTOS else "depth planes only"
        print(f"{self.LABEL} pool: {self.pool.n} pairs ({planes}), frames of {fh}x{fw} inside the border box, "
              f"{self.pool.nbytes / 2 ** 20:.1f} MiB resident in device memory")

    def draw(self):
        """(idx, top, left, flip) of one batch, int32 device tensors.  ``split: test``: the next ``batch`` pairs in order (wrapping),
        the frame's own corner, no flip."""
        if self.test:
            idx = (torch.arange(self.batch, device=self.device) + self._cursor) % self.pool.n
            self._cursor = (self._cursor + self.batch) % self.pool.n
            return idx.to(torch.int32), self._zeros, self._zeros, self._zeros
        idx = self.take_indices()
        r = torch.randint(0, 2 ** 31 - 1, (2, self.batch), device=self.device, generator=self.gen)
        return idx.to(torch.int32), (r[0] % self._span[0]).to(torch.int32), (r[1] % self._span[1]).to(torch.int32), self.draw_flip()

    def next_batch(self, idx=None, top=None, left=None, flip=None):
        host_idx = None
        if self.test:          # names need the indices on the host; a test walk knows them without a read-back
            host_idx = [(self._cursor + i) % self.pool.n for i in range(self.batch)] if idx is None else [int(i) for i in idx]
        if idx is None or top is None or left is None or flip is None:
            if self.test and idx is not None:
                d = (None, self._zeros[:len(host_idx)], self._zeros[:len(host_idx)], self._zeros[:len(host_idx)])
            else:
                d = self.draw()
            idx, top, left, flip = (g if v is None else v for v, g in zip((idx, top, left, flip), d))
        image, cond = depth_batch(self.pool, idx, top, left, flip, self.size, True, self.PHOTOS)
        out = {"image": image}
        if self.PHOTOS:
            out["cond"] = cond
        if host_idx is not None:
            n = self.pool.n
            out["img_name"] = [self.names[min(max(i, 0), n - 1)] for i in host_idx]
            out["ori_size"] = [self.ori_sizes[min(max(i, 0), n - 1)] for i in host_idx]
        return out

    def __next__(self):
        return self.next_batch()


class DepthMapStream(DepthBatchStream):
    """The first-stage source of the depth recipe: {'image': depth [B,1,H,W]} only, the same pool layout and draws.  On real data the
    photos are located (a depth file is found through its photo) but never decoded, and no photo pool exists."""

    PHOTOS = False
    LABEL = "depth map"
    channels = 1
