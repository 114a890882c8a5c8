"""Saliency and sketch-to-image training pairs on the HIP hot path: the batches of ``ddm.data.DUTSDataset`` (ddm/data.py:953-1026 of
the reference) and ``ddm.data.SketchDataset`` (:1028-1103) made by one kernel launch from two uint8 pools resident in device memory.

The reference makes each pair on the host with PIL: the RGB photo and its grey ground-truth map are opened [:1002-1004], both
resized to ``image_size`` with the antialiased bilinear filter [:982-983, Resize -> F.resize -> Image.resize], flipped with one
draw [:984], and returned as ``{'image': map [1,H,W], 'cond': photo [3,H,W]}`` in [-1, 1] [:1019-1026].  The sources differ in
size from sample to sample -- and the map need not have its photo's size -- so every sample has its own four 1-D resize tables.
A table depends on (in_size, out_size) only: ``build_table_pool`` makes one per distinct source width and height with
``sr_data.resample_table`` and concatenates them into one int32 table pool with a directory;
``adm_pair_resize_batch`` (adm_amd/csrc/pair_data.hip) looks a sample's tables up through its image index and runs PIL's integer
two-pass arithmetic, so the bytes are PIL's.  No floating-point coefficient arithmetic happens on the device.

``DUTSBatchStream`` and ``SketchBatchStream`` (the same pool and draws with the roles of the two planes exchanged: the photo is the
``image``, the one-channel sketch the ``cond``) are batch sources of train_cond_ldm.py and, with ``split: test``, of
sample_cond_ldm.py.  The draws live on the
device: no ``.item()`` / ``.cpu()`` and no dataloader workers on the per-step path.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import hip
from ..hip import call, ptr
from .sr_data import PoolStream, _draw, pack_bytes, resample_table

LDS_BUDGET = 64 * 1024          # kLdsBudget of adm_amd/csrc/resample_u8.h
DUTS_CLASSES = ("ddm.data.DUTSDataset", "DUTSDataset")
SPLIT_DIRS = {"train": "DUTS-TR", "test": "DUTS-TE"}          # data.py:964-967
SKETCH_CLASSES = ("ddm.data.SketchDataset", "SketchDataset")
SKETCH_SPLIT_DIRS = {"train": "train", "test": "val"}         # data.py:1039-1042


def table_pool(axes) -> Dict[str, np.ndarray]:
    """The table pool of ``axes`` = [N][A] pairs (in_size, out_size), the 1-D resizes of each of N images: ``tab`` int32 (table t =
    bounds [out][2] then coefficients [out][k], flattened), ``dir`` int32 [T, 2] = {offset, k}, ``img_tab`` int32 [N, A] = the table id
    of every pair, and ``keys`` = [(in, out)] per table.  Equal pairs share one table, whichever axis, plane or image they come
    from; ids are given in the order of first use."""
    ids: Dict[Tuple[int, int], int] = {}
    parts, directory, total = [], [], 0

    def table(in_size, out_size):
        nonlocal total
        key = (int(in_size), int(out_size))
        if key not in ids:
            bounds, coeffs = resample_table(key[0], key[1], "bilinear")
            ids[key] = len(directory)
            directory.append((total, coeffs.shape[1]))
            parts.extend((bounds.reshape(-1), coeffs.reshape(-1)))
            total += bounds.size + coeffs.size
        return ids[key]

    img_tab = np.asarray([[table(i, o) for i, o in row] for row in axes], dtype=np.int32)
    return {"tab": np.concatenate(parts).astype(np.int32), "dir": np.asarray(directory, dtype=np.int32).reshape(-1, 2),
            "img_tab": img_tab.reshape(len(axes), -1), "keys": list(ids)}


def build_table_pool(rgb_hw, gray_hw, out_hw) -> Dict[str, np.ndarray]:
    """The ``table_pool`` of resizing every source size in ``rgb_hw`` / ``gray_hw`` ([N, 2] = (height, width)) to ``out_hw``:
    ``img_tab`` int32 [N, 4] = ids of {photo width, photo height, map width, map height}."""
    H, W = int(out_hw[0]), int(out_hw[1])
    rgb_hw, gray_hw = np.asarray(rgb_hw).reshape(-1, 2), np.asarray(gray_hw).reshape(-1, 2)
    if rgb_hw.shape != gray_hw.shape:
        raise ValueError(f"{rgb_hw.shape[0]} photos but {gray_hw.shape[0]} maps")
    return table_pool([[(r[1], W), (r[0], H), (g[1], W), (g[0], H)] for r, g in zip(rgb_hw.tolist(), gray_hw.tolist())])


def read_table(pool: Dict[str, np.ndarray], t: int, out_size: int):
    """(bounds [out, 2], coeffs [out, k]) of table ``t``: the directory read back."""
    off, k = (int(v) for v in pool["dir"][t])
    flat = pool["tab"][off:off + out_size * (2 + k)]
    return flat[:2 * out_size].reshape(out_size, 2), flat[2 * out_size:].reshape(out_size, k)


def taps(in_size: int, out_size: int) -> int:
    """Longest window of the bilinear table in_size -> out_size, without building it (PIL: ceil(support) * 2 + 1)."""
    return int(math.ceil(max(float(in_size) / out_size, 1.0))) * 2 + 1


def lds_need(out_hw, max_h: int, max_w: int) -> int:
    """LDS bytes of a tile whose sources are at most max_h x max_w (the C ABI's own figure)."""
    H, W = int(out_hw[0]), int(out_hw[1])
    return int(hip.lib().adm_pair_resize_lds(H, W, int(max_h), int(max_w), taps(max_w, W), taps(max_h, H)))


def check_sizes(sizes, out_hw, label, what) -> Tuple[int, int]:
    """The budget rule of every pool of ragged sources: refuse a source ``sizes[i]`` = (height, width) whose ratio to the target
    needs more LDS than a workgroup has, and a tallest and a widest source that fit one by one but not together (the capacity is
    sized once, from both).  ``label(i)`` names entry i, ``what(i)`` says what it is ('its photo is', 'it is').  Returns
    (max_h, max_w)."""
    H, W = int(out_hw[0]), int(out_hw[1])
    sizes = np.asarray(sizes).reshape(-1, 2)
    need = {}
    for i, (h, w) in enumerate(sizes.tolist()):
        if (h, w) not in need:
            need[(h, w)] = lds_need(out_hw, h, w)
        if need[(h, w)] > LDS_BUDGET:
            raise ValueError(f"{label(i)}: {what(i)} {h}x{w}, {h / H:.2f} x {w / W:.2f} times the "
                             f"{H}x{W} target; its tile needs {need[(h, w)]} bytes of LDS, the budget is {LDS_BUDGET} (ratios up to "
                             "about 7 per axis fit)")
    max_h, max_w = int(sizes[:, 0].max()), int(sizes[:, 1].max())
    if lds_need(out_hw, max_h, max_w) > LDS_BUDGET:
        ih, iw = int(sizes[:, 0].argmax()), int(sizes[:, 1].argmax())
        raise ValueError(f"{label(ih)} ({max_h} rows) and {label(iw)} ({max_w} columns) together need "
                         f"{lds_need(out_hw, max_h, max_w)} bytes of LDS for the {H}x{W} target, the budget is {LDS_BUDGET}")
    return max_h, max_w


def check_budget(rgb_hw, gray_hw, out_hw, names: Optional[Sequence[str]] = None) -> Tuple[int, int]:
    """Refuse, by name, a pair whose source-to-target ratio needs more LDS than a workgroup has; returns (max_h, max_w)."""
    sizes = np.concatenate([np.asarray(rgb_hw).reshape(-1, 2), np.asarray(gray_hw).reshape(-1, 2)])
    n = len(sizes) // 2
    label = (lambda i: f"pair {i % n} ({names[i % n]})") if names else (lambda i: f"pair {i % n}")
    return check_sizes(sizes, out_hw, label, lambda i: f"its {'photo' if i < n else 'map'} is")


class PairPool:
    """The two packed pools (3 bytes and 1 byte per pixel), their per-image tables and the table pool, in device memory."""

    def __init__(self, rgb_flat, rgb_off, rgb_hw, gray_flat, gray_off, gray_hw, out_hw, device, names=None):
        """*_flat: uint8 device tensors (a multiple of 4 bytes); *_off int64 [N] / *_hw int32 [N, 2]: host arrays."""
        self.out_hw = (int(out_hw[0]), int(out_hw[1]))
        self.names = list(names) if names is not None else None
        self.hw_host = (np.asarray(rgb_hw, dtype=np.int32).reshape(-1, 2), np.asarray(gray_hw, dtype=np.int32).reshape(-1, 2))
        self.n = int(self.hw_host[0].shape[0])
        self.max_h, self.max_w = check_budget(*self.hw_host, self.out_hw, self.names)
        self.kh, self.kv = taps(self.max_w, self.out_hw[1]), taps(self.max_h, self.out_hw[0])
        self.tables = build_table_pool(*self.hw_host, self.out_hw)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.rgb, self.gray = rgb_flat, gray_flat
        self.rgb_off, self.gray_off = dev(np.asarray(rgb_off, dtype=np.int64)), dev(np.asarray(gray_off, dtype=np.int64))
        self.rgb_hw, self.gray_hw = dev(self.hw_host[0]), dev(self.hw_host[1])
        self.tab, self.tab_dir, self.img_tab = dev(self.tables["tab"]), dev(self.tables["dir"]), dev(self.tables["img_tab"])

    @classmethod
    def from_arrays(cls, photos: Sequence[np.ndarray], maps: Sequence[np.ndarray], out_hw, device, names=None) -> "PairPool":
        """photos: uint8 [H,W,3]; maps: uint8 [H,W] (sizes may differ, also between a photo and its map)."""
        if len(photos) != len(maps):
            raise ValueError(f"{len(photos)} photos but {len(maps)} maps")
        rf, ro, rh = pack_bytes(photos, 3, "photo")
        gf, go, gh = pack_bytes(maps, 1, "map")
        check_budget(rh, gh, out_hw, names)          # before anything is copied to the device
        return cls(torch.from_numpy(rf).to(device), ro, rh, torch.from_numpy(gf).to(device), go, gh, out_hw, device, names)

    @classmethod
    def from_uniform_draws(cls, sizes: Sequence[Tuple[int, int]], out_hw, device, gen) -> "PairPool":
        """U(0,255) bytes drawn on the device for pairs of the given (height, width) sizes."""
        hw = np.asarray(sizes, dtype=np.int32).reshape(-1, 2)
        px = hw[:, 0].astype(np.int64) * hw[:, 1]
        off = np.concatenate([[0], np.cumsum(px)[:-1]]).astype(np.int64)
        flat = lambda nbytes: torch.randint(0, 256, ((int(nbytes) + 3) // 4 * 4,), device=device, dtype=torch.uint8, generator=gen)
        return cls(flat(3 * px.sum()), 3 * off, hw, flat(px.sum()), off, hw, out_hw, device)

    @property
    def nbytes(self) -> int:
        return int(self.rgb.numel() + self.gray.numel() + 4 * self.tab.numel())


def launch(pool: PairPool, idx, flip, rgb, gray, rgb_u8, gray_u8, B: int):
    """The raw ``adm_pair_resize_batch`` call on buffers the caller owns."""
    H, W = pool.out_hw
    call("adm_pair_resize_batch", ptr(pool.rgb), pool.rgb.numel(), ptr(pool.rgb_off), ptr(pool.rgb_hw), ptr(pool.gray),
         pool.gray.numel(), ptr(pool.gray_off), ptr(pool.gray_hw), pool.n, ptr(pool.tab), pool.tab.numel(), ptr(pool.tab_dir),
         int(pool.tab_dir.shape[0]), ptr(pool.img_tab), pool.max_h, pool.max_w, pool.kh, pool.kv, ptr(idx), ptr(flip), ptr(rgb),
         ptr(gray), ptr(rgb_u8), ptr(gray_u8), B, H, W)


@torch.no_grad()
def pair_batch(pool: PairPool, idx, flip, want_u8: bool = False):
    """One ``adm_pair_resize_batch`` launch: (rgb [B,3,H,W], gray [B,1,H,W], rgb_u8 [B,H,W,3] or None, gray_u8 [B,H,W] or None)
    for the draws idx / flip (int32 [B] device tensors; anything else is converted)."""
    hip.require_cuda(pool.rgb, "the photo pool")
    dev = pool.rgb.device
    B = int(torch.as_tensor(idx).numel())
    idx, flip = _draw(idx, B, dev), _draw(flip, B, dev)
    H, W = pool.out_hw
    rgb = torch.empty(B, 3, H, W, device=dev, dtype=torch.float32)
    gray = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32)
    rgb_u8 = torch.empty(B, H, W, 3, device=dev, dtype=torch.uint8) if want_u8 else None
    gray_u8 = torch.empty(B, H, W, device=dev, dtype=torch.uint8) if want_u8 else None
    launch(pool, idx, flip, rgb, gray, rgb_u8, gray_u8, B)
    return rgb, gray, rgb_u8, gray_u8


def find_duts_pairs(data_root: str, split: str = "train"):
    """[(photo path, map path)] sorted by photo path: the reference's discovery (data.py:964-980) -- ``DUTS-TR`` / ``DUTS-TE`` below
    ``data_root`` by ``split`` (any other split: ``data_root`` itself), every ``*.jpg`` found recursively, its map at
    ``parent.parent / parent.name.replace('Image', 'Mask') / name.replace('.jpg', '.png')``.  A missing map raises and names it (the
    reference would draw another index at run time, :1006-1007)."""
    from pathlib import Path
    folder = Path(data_root) / SPLIT_DIRS[split] if split in SPLIT_DIRS else Path(data_root)
    photos = sorted(folder.rglob("*.jpg"))
    if not photos:
        raise FileNotFoundError(f"data.data_root: no jpg photo below {folder}")
    pairs = []
    for p in photos:
        m = p.parent.parent / p.parent.name.replace("Image", "Mask") / p.name.replace(".jpg", ".png")
        if not m.exists():
            raise FileNotFoundError(f"the ground-truth map of {p} is missing: {m}")
        pairs.append((p, m))
    return pairs


def load_duts(data_root: str, split: str = "train"):
    """(photos uint8 [H,W,3], maps uint8 [H,W], photo file names): decoded once with PIL, ``.convert('RGB')`` / ``.convert('L')``
    (data.py:1002-1004)."""
    from PIL import Image
    pairs = find_duts_pairs(data_root, split)
    photos = [np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8) for p, _ in pairs]
    maps = [np.asarray(Image.open(m).convert("L"), dtype=np.uint8) for _, m in pairs]
    return photos, maps, [p.name for p, _ in pairs]


def synthetic_sizes(out_hw, n: int) -> List[Tuple[int, int]]:
    """A few sizes around ``out_hw``, smaller and larger, so that up-scaling, identity and down-scaling tables all run."""
    H, W = int(out_hw[0]), int(out_hw[1])
    kinds = [(H - H // 4, W - W // 8), (H, W + W // 4), (H + H // 8, W), (H + H // 3, W + W // 2), (H - H // 8, W + W // 8)]
    return [kinds[i % len(kinds)] for i in range(n)]


class PairBatchStream(PoolStream):
    """Infinite iterator of (RGB, grey) pair batches in [-1, 1] on the GPU from a ``PairPool``: what the saliency and the
    sketch-to-image streams share.  A subclass names its dataset (``CLASSES``, ``LABEL``), loads its files (``load``) and says which
    plane is the batch's ``image`` and which its ``cond`` (``ROLES`` = the keys of (rgb, grey)).

    ``split: train`` draws the image order as SRBatchStream does (a fresh permutation per epoch, continued across the boundary) and the
    flip with p = 0.5 when ``augment_horizontal_flip``.  ``split: test`` walks the pairs in sorted order without flips and its
    batches carry ``img_name`` and ``ori_size`` = [(h, w)] of the photos; ``names`` / ``ori_sizes`` hold them for the whole pool.
    ``next_batch(idx=, flip=)`` accepts injected draws."""

    SYNTHETIC_PAIRS = 32
    CLASSES: Tuple[str, ...] = ()
    LABEL = ""
    ROLES = ("cond", "image")
    SYNTHETIC_NAME = "{:010d}.png"

    @staticmethod
    def load(data_root: str, split: str):
        raise NotImplementedError

    def __init__(self, data_cfg, batch, image_size, device, seed):
        data_cfg = data_cfg or {}
        full = self.CLASSES[0]
        self.split = data_cfg.get("split") or "train"
        if self.split not in ("train", "test"):
            raise NotImplementedError(f"data.split {self.split!r}: {full}.__getitem__ raises for anything but 'train' / 'test'")
        train = self.split == "train"
        super().__init__(batch, device, seed, train and bool(data_cfg.get("augment_horizontal_flip", False)))
        self.size = (int(image_size[0]), int(image_size[1]))
        cls = data_cfg.get("class_name")
        if cls in self.CLASSES:
            if not data_cfg.get("data_root"):
                raise ValueError(f"data.class_name {full} needs data.data_root")
            photos, maps, names = self.load(data_cfg.get("data_root"), self.split)
            self.pool = PairPool.from_arrays(photos, maps, self.size, device, names)
        elif cls == "synthetic" and data_cfg.get("synthetic_of") in self.CLASSES:
            self.pool = PairPool.from_uniform_draws(synthetic_sizes(self.size, self.SYNTHETIC_PAIRS), self.size, device, self.gen)
        else:
            raise NotImplementedError(f"data.class_name {cls!r}: only {full} + data_root, or 'synthetic' with "
                                      f"synthetic_of: {full} (U(0,255) pairs, benchmarking only) are implemented")
        self.names = self.pool.names or [self.SYNTHETIC_NAME.format(i) for i in range(self.pool.n)]
        self.ori_sizes = [(int(h), int(w)) for h, w in self.pool.hw_host[0]]
        self._cursor = 0          # split: test
        print(f"{self.LABEL} pool: {self.pool.n} pairs, {len(self.pool.tables['keys'])} resize tables, "
              f"{self.pool.nbytes / 2 ** 20:.1f} MiB resident in device memory")

    def draw(self):
        """(idx, flip) of one batch, int32 device tensors.  ``split: test``: the next ``batch`` pairs in order (wrapping), no flip."""
        if self.split == "test":
            idx = (torch.arange(self.batch, device=self.device) + self._cursor) % self.pool.n
            self._cursor = (self._cursor + self.batch) % self.pool.n
            return idx.to(torch.int32), self._zeros
        return self.take_indices().to(torch.int32), self.draw_flip()

    def next_batch(self, idx=None, flip=None, want_u8: bool = False):
        host_idx = None
        if self.split == "test":          # names need the indices on the host; a test walk knows them without a read-back
            host_idx = [(self._cursor + i) % self.pool.n for i in range(self.batch)] if idx is None else [int(i) for i in idx]
        if idx is None or flip is None:
            d = self.draw()
            idx, flip = (g if v is None else v for v, g in zip((idx, flip), d))
        rgb, gray, rgb_u8, gray_u8 = pair_batch(self.pool, idx, flip, want_u8)
        k_rgb, k_gray = self.ROLES
        planes = {k_rgb: (rgb, rgb_u8), k_gray: (gray, gray_u8)}
        out = {k: planes[k][0] for k in ("image", "cond")}          # 'image' first, as both datasets key their samples
        if want_u8:
            out.update({k + "_u8": planes[k][1] for k in ("image", "cond")})
        if host_idx is not None:
            n = self.pool.n
            out["img_name"] = [self.names[min(max(i, 0), n - 1)] for i in host_idx]
            out["ori_size"] = [self.ori_sizes[min(max(i, 0), n - 1)] for i in host_idx]
        return out

    def __next__(self):
        return self.next_batch()


class DUTSBatchStream(PairBatchStream):
    """{'image': map [B,1,H,W], 'cond': photo [B,3,H,W]}, keyed in the order ddm.data.DUTSDataset keys them (data.py:1026).

    Sources, in this order: ``data.class_name: ddm.data.DUTSDataset`` + ``data_root`` (``find_duts_pairs``; decoded once at start-up
    into the two packed pools); ``data.class_name: synthetic`` with ``synthetic_of: ddm.data.DUTSDataset`` (U(0,255) pools drawn on the
    device, of a few sizes around ``image_size``).  Anything else raises.  Splits as in data.py:987-991, 1013-1018."""

    CLASSES = DUTS_CLASSES
    LABEL = "DUTS"
    ROLES = ("cond", "image")
    SYNTHETIC_NAME = "{: 010d}.jpg"
    load = staticmethod(load_duts)


def find_sketch_pairs(data_root: str, split: str = "train"):
    """[(photo path, sketch path)] sorted by photo path: the reference's discovery (data.py:1039-1057) -- every ``*.png`` below
    ``data_root/GT/{train|val}`` (``split: test`` reads ``val``; any other split: ``data_root`` itself) whose name does not start
    with ``._``, its sketch at the same relative path below the sibling tree ``Sketch``.  DEVIATION: a missing sketch raises here and
    names the file; the reference substitutes a random other sample at run time (:1074-1084)."""
    from pathlib import Path
    root = Path(data_root)
    if split in SKETCH_SPLIT_DIRS:
        folder, sketches = root / "GT" / SKETCH_SPLIT_DIRS[split], root / "Sketch" / SKETCH_SPLIT_DIRS[split]
    else:          # the reference's own rule for a bare folder: .../GT/<split>/<class>/<name> -> .../Sketch/<split>/<class>/<name>
        folder, sketches = root, None
    photos = sorted(p for p in folder.rglob("*.png") if not p.name.startswith("._"))
    if not photos:
        raise FileNotFoundError(f"data.data_root: no png photo below {folder}")
    pairs = []
    for p in photos:
        if sketches is not None:
            s = sketches / p.relative_to(folder)
        else:
            top = p.parent.parent.parent
            s = top.parent / top.name.replace("GT", "Sketch") / p.parent.parent.name / p.parent.name / p.name
        if not s.is_file():
            raise FileNotFoundError(f"the sketch of {p} is missing: {s}")
        pairs.append((p, s))
    return pairs


def load_sketch(data_root: str, split: str = "train"):
    """(photos uint8 [H,W,3], sketches uint8 [H,W], photo file names): decoded once with PIL, ``.convert('RGB')`` / ``.convert('L')``
    (data.py:1079-1081).  An unreadable file raises and names itself."""
    from PIL import Image
    photos, sketches, names = [], [], []
    for p, s in find_sketch_pairs(data_root, split):
        for path, mode, dst in ((p, "RGB", photos), (s, "L", sketches)):
            try:
                dst.append(np.asarray(Image.open(path).convert(mode), dtype=np.uint8))
            except Exception as e:
                raise OSError(f"{path} cannot be read as an image: {e}") from e
        names.append(p.name)
    return photos, sketches, names


class SketchBatchStream(PairBatchStream):
    """{'image': photo [B,3,H,W], 'cond': sketch [B,1,H,W]}, keyed as ddm.data.SketchDataset keys them (data.py:1103): the
    sketch-to-image recipe GENERATES the photo, so the roles are the opposite of the saliency stream's.

    Sources: ``data.class_name: ddm.data.SketchDataset`` + ``data_root`` (``find_sketch_pairs``), or ``class_name: synthetic`` with
    ``synthetic_of: ddm.data.SketchDataset``.  Both planes are resized to ``image_size`` with PIL's antialiased bilinear filter and
    flipped with one draw (data.py:1059-1063, 1090-1093) by ``adm_pair_resize_batch``."""

    CLASSES = SKETCH_CLASSES
    LABEL = "sketch"
    ROLES = ("image", "cond")
    load = staticmethod(load_sketch)
