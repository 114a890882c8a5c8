"""numpy restatement of PIL's 8-bit Image.resize (ImagingResample: coefficients with 22 fractional bits, horizontal pass clipped
to uint8, vertical pass over that) and of the steps of ddm.data.SRDataset / SRDatasetTest built on it.  TEST INFRASTRUCTURE ONLY:
the reference for fresh inputs where PIL may be absent; tests/test_sr_data_host.py pins it against PIL's own bytes
(tests/golden/g21_sr_data.npz).  Written independently of adm_amd/ddm/sr_data.py (vectorised, its own coefficient code)."""
import numpy as np
import torch

from oracle import fill


def hash_bytes(shape, tag):
    """Deterministic uint8 array (oracle.fill's integer hash): reproducible on any machine."""
    v = (fill.hash_tensor(tuple(shape), tag, 1.0, torch.float64).numpy() + 1.0) * 128.0
    return np.clip(np.floor(v), 0, 255).astype(np.uint8)


def _weights(x, kind):
    x = np.abs(x)
    if kind == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    if kind == "bicubic":
        a = -0.5
        return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))
    raise NotImplementedError(kind)


def coeffs(in_size, out_size, kind):
    """[(start, int32 weights)] per output coordinate."""
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = {"bilinear": 1.0, "bicubic": 2.0}[kind] * fscale
    out = []
    for i in range(out_size):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        w = _weights((np.arange(lo, hi) - center + 0.5) * (1.0 / fscale), kind)
        total = 0.0
        for v in w:          # PIL sums in running order
            total += float(v)
        w = w / total
        out.append((lo, np.where(w < 0, -0.5 + w * 4194304.0, 0.5 + w * 4194304.0).astype(np.int64)))      # astype truncates
    return out


def _pass(img, table):
    """Resample axis 1 of uint8 [R, C, 3]."""
    res = np.empty((img.shape[0], len(table), 3), dtype=np.uint8)
    for i, (lo, k) in enumerate(table):
        acc = (1 << 21) + np.tensordot(img[:, lo:lo + len(k)].astype(np.int64), k, axes=([1], [0]))
        assert np.abs(acc).max() < 2 ** 31          # the kernel's int32 accumulator holds it
        res[:, i] = np.clip(acc >> 22, 0, 255)
    return res


def resize_u8(img, out_hw, kind="bicubic", stats=None):
    """uint8 [H, W, 3] -> uint8 [h, w, 3].  stats (a dict) receives how many horizontal-pass values were clipped."""
    H, W = img.shape[:2]
    h, w = out_hw
    tab = coeffs(W, w, kind)
    if stats is not None:
        n = 0
        for lo, k in tab:
            v = ((1 << 21) + np.tensordot(img[:, lo:lo + len(k)].astype(np.int64), k, axes=([1], [0]))) >> 22
            n += int(((v < 0) | (v > 255)).sum())
        stats["horizontal_clipped"] = n
    hor = _pass(img, tab)
    return _pass(hor.transpose(1, 0, 2), coeffs(H, h, kind)).transpose(1, 0, 2)


def sr_pair(img, top, left, size, down=4, kind="bicubic", flip=False):
    """SRDataset.__getitem__ on bytes: (crop uint8 [H, W, 3], cond uint8 [H/down, W/down, 3]), both flipped when `flip`."""
    H, W = size
    crop = img[top:top + H, left:left + W]
    cond = resize_u8(crop, (H // down, W // down), kind)
    if flip:
        crop, cond = crop[:, ::-1], cond[:, ::-1]
    return np.ascontiguousarray(crop), np.ascontiguousarray(cond)


def sr_test_pair(img, down=4, kind="bicubic"):
    """SRDatasetTest.__getitem__ on bytes: (the unpadded image, cond of the image padded with black to multiples of 256)."""
    H, W = img.shape[:2]
    Hp, Wp = -(-H // 256) * 256, -(-W // 256) * 256
    pad = np.zeros((Hp, Wp, 3), dtype=np.uint8)
    pad[:H, :W] = img
    return img, resize_u8(pad, (Hp // down, Wp // down), kind)


def to_float(u8):
    """uint8 [..., H, W, 3] -> float32 [..., 3, H, W]: ToTensor then *2-1, as torch computes it on the CPU."""
    t = torch.from_numpy(np.ascontiguousarray(u8))
    return (t.float() / 255 * 2 - 1).movedim(-1, -3).contiguous()
