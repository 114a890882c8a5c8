"""GPU: super-resolution batches made by adm_sr_batch (adm_amd/csrc/sr_data.hip) against PIL's own bytes
(tests/golden/g21_sr_data.npz) and, for fresh inputs, against tests/sr_data_ref.py (which tests/test_sr_data_host.py pins to
the same golden file).  Every case asserts: `cond_u8` equals the expected bytes with ZERO mismatches (the arithmetic is integer:
a condition, not a tolerance); round((cond + 1) * 127.5) gives the same bytes; `image` and `cond` equal the CPU's
u8.float() / 255 * 2 - 1 within 5e-7 (values in [-1, 1], f32 eps 6e-8: room for a division done by reciprocal, <= 2 ulp, and
nothing coarser)."""
import os

import numpy as np
import pytest
import torch

import sr_data_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_sr_data.npz")
FLOAT_TOL = 5e-7


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def check(image, cond, cond_u8, want_image, want_cond):
    """want_image uint8 [B,H,W,3] / want_cond uint8 [B,h,w,3]: the three assertions of the module docstring."""
    want_image, want_cond = np.ascontiguousarray(want_image), np.ascontiguousarray(want_cond)
    got_u8 = cond_u8.cpu().numpy()
    assert got_u8.shape == want_cond.shape and got_u8.dtype == np.uint8
    wrong = int((got_u8 != want_cond).sum())
    rounded = torch.round((cond.cpu() + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    wrong_rounded = int((rounded != want_cond).sum())
    e_cond = float((cond.cpu() - R.to_float(want_cond)).abs().max())
    e_image = float((image.cpu() - R.to_float(want_image)).abs().max())
    print(f"cond_u8 mismatches {wrong}, rounded-cond mismatches {wrong_rounded}, max |cond - cpu| {e_cond:.2e}, "
          f"max |image - cpu| {e_image:.2e}")
    assert image.dtype == torch.float32 and cond.dtype == torch.float32
    assert tuple(image.shape) == (want_image.shape[0], 3) + want_image.shape[1:3]
    assert wrong == 0
    assert wrong_rounded == 0
    assert e_cond <= FLOAT_TOL and e_image <= FLOAT_TOL


def run(gpu, images, size, out_size, kind, idx, top, left, flip):
    from adm_amd.ddm.sr_data import ImagePool, Resampler, sr_batch
    pool = ImagePool.from_arrays(images, size, gpu)
    out = sr_batch(pool, Resampler(size, out_size, kind, gpu), idx, top, left, flip, want_u8=True)
    torch.cuda.synchronize()
    return out


def test_clipped_windows(gpu, g):
    """16x16, the crop is the whole image, /4: no interior window exists, every window is clipped by a border."""
    x = g["clipped.in"]
    check(*run(gpu, [x], (16, 16), (4, 4), "bicubic", [0], [0], [0], [0]), g["clipped.image"][None], g["clipped.cond"][None])


def test_ragged_pool_crops_and_flips(gpu, g):
    """Three images of different sizes (80x72, 64x48, 100x65: a width not divisible by 4), B = 3, crop 64x48 -> 16x12: one index
    used twice with different offsets, offsets 0 and the maximum, flips 0 and 1, H != W, the per-image offset table."""
    d = g["pool.draws"]
    assert d[0, 0] == d[2, 0] and (d[0, 1], d[0, 2]) != (d[2, 1], d[2, 2]) and set(d[:, 3].tolist()) == {0, 1}
    assert d[0, 1] == 0 and d[1, 2] == 0 and d[0, 2] == 72 - 48 and d[1, 1] == 100 - 64 and d[2, 1] == 80 - 64
    images = [g[f"pool.in{i}"] for i in range(3)]
    check(*run(gpu, images, (64, 48), (16, 12), "bicubic", d[:, 0], d[:, 1], d[:, 2], d[:, 3]), g["pool.image"], g["pool.cond"])


def test_uint8_intermediate(gpu, g):
    """32x32 step edges (half-planes of 0 / 255, another per channel) -> 8x8.  On the CPU 116 horizontal-pass values fall outside
    [0, 255] before the clip, and 76 / 85 output bytes sit at 0 / 255 (tests/test_sr_data_host.py), so a float intermediate or
    a missing clip cannot pass."""
    want = g["edge.cond"]
    assert int((want == 0).sum()) > 0 and int((want == 255).sum()) > 0
    stats = {}
    R.resize_u8(g["edge.in"], (8, 8), "bicubic", stats)
    assert stats["horizontal_clipped"] > 0
    check(*run(gpu, [g["edge.in"]], (32, 32), (8, 8), "bicubic", [0], [0], [0], [0]), g["edge.image"][None], want[None])


@pytest.mark.parametrize("tag", ["nonint", "by8", "bilinear"])
def test_table_generality(gpu, g, tag):
    """36x28 -> 12x9 (non-integer scale, bicubic), 24x40 -> 3x5 (/8), 32x48 -> 8x12 bilinear: nothing assumes a factor of 4."""
    x, want, kind = g[f"{tag}.in"], g[f"{tag}.cond"], str(g[f"{tag}.kind"])
    check(*run(gpu, [x], x.shape[:2], want.shape[:2], kind, [0], [0], [0], [0]), x[None], want[None])


def test_several_tiles(gpu):
    """One crop whose low-resolution size is two workgroup tiles plus a ragged remainder in both directions; the size is derived
    from the tile constants the binding exports (adm_sr_tile), so it follows a change of the tile.  Flipped, at an offset."""
    from adm_amd import hip
    th, tw = hip.lib().adm_sr_tile(0), hip.lib().adm_sr_tile(1)
    assert th > 0 and tw > 0
    h, w = 2 * th + 5, 2 * tw + 3
    H, W = 4 * h, 4 * w
    x = R.hash_bytes((H + 3, W + 5, 3), "sr.tiles")
    image, cond = R.sr_pair(x, 2, 5, (H, W), flip=True)
    check(*run(gpu, [x], (H, W), (h, w), "bicubic", [0], [2], [5], [1]), image[None], cond[None])


def test_fresh_data_at_the_recipe_shape(gpu):
    """B = 2, 512x512 -> 128x128 from hashed bytes, one sample flipped."""
    from adm_amd.ddm.sr_data import ImagePool, Resampler, sr_batch
    x = R.hash_bytes((2, 512, 512, 3), "sr.recipe")
    pool = ImagePool.from_uniform(torch.from_numpy(x).to(gpu), (512, 512))
    out = sr_batch(pool, Resampler((512, 512), (128, 128), "bicubic", gpu), [1, 0], [0, 0], [0, 0], [0, 1], want_u8=True)
    pairs = [R.sr_pair(x[1], 0, 0, (512, 512)), R.sr_pair(x[0], 0, 0, (512, 512), flip=True)]
    check(*out, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))


def test_unsupported_shape_is_refused_without_a_launch(gpu):
    """/16 bicubic needs a source rectangle beyond the LDS budget: the wrapper returns its error code, as its neighbours do."""
    x = R.hash_bytes((1024, 1024, 3), "sr.big")
    with pytest.raises(RuntimeError, match="adm_sr_batch failed with code -22"):
        run(gpu, [x], (1024, 1024), (64, 64), "bicubic", [0], [0], [0], [0])


def _stream(gpu, tmp_path, batch, seed=7, **kw):
    from adm_amd.ddm.sr_data import SRBatchStream
    path = str(tmp_path / "pool.npy")
    if not os.path.exists(path):
        np.save(path, R.hash_bytes((5, 40, 36, 3), "sr.stream"))
    return SRBatchStream({"npy": path, "augment_horizontal_flip": True, **kw}, batch, (32, 32), gpu, seed), np.load(path)


def test_stream_draws(gpu, tmp_path):
    a, x = _stream(gpu, tmp_path, 2)
    b, _ = _stream(gpu, tmp_path, 2)
    for _ in range(3):          # the same seed gives the same batches
        ba, bb = next(a), next(b)
        assert list(ba) == ["image", "cond"] and torch.equal(ba["image"], bb["image"]) and torch.equal(ba["cond"], bb["cond"])
    assert tuple(ba["image"].shape) == (2, 3, 32, 32) and tuple(ba["cond"].shape) == (2, 3, 8, 8)
    # two epochs of the 5-image pool in full batches of 2: every index exactly twice; offsets in range
    s, _ = _stream(gpu, tmp_path, 2, seed=8)
    draws = [s.draw() for _ in range(5)]
    idx = torch.cat([d[0] for d in draws]).cpu()
    assert sorted(idx.tolist()) == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    assert sorted(idx[:5].tolist()) == [0, 1, 2, 3, 4]          # the first epoch is one permutation
    top, left = torch.cat([d[1] for d in draws]).cpu(), torch.cat([d[2] for d in draws]).cpu()
    assert int(top.min()) >= 0 and int(top.max()) <= 40 - 32 and int(left.min()) >= 0 and int(left.max()) <= 36 - 32
    # a drawn batch is what the reference makes of its draws
    i, t, l, f = s.draw()
    out = s.next_batch(idx=i, top=t, left=l, flip=f, want_u8=True)
    pairs = [R.sr_pair(x[int(i[k])], int(t[k]), int(l[k]), (32, 32), flip=bool(f[k])) for k in range(2)]
    check(out["image"], out["cond"], out["cond_u8"], np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
    # flips: p = 0.5.  4096 draws: sigma = 0.5 / 64 = 0.0078, so 0.5 +- 0.04 is 5 sigma: a fair coin stays inside it
    s, _ = _stream(gpu, tmp_path, 256, seed=9)
    flips, tops, lefts = zip(*[(d[3], d[1], d[2]) for d in (s.draw() for _ in range(16))])
    freq = float(torch.cat(flips).float().mean())
    print(f"flip frequency over 4096 draws: {freq:.4f}")
    assert abs(freq - 0.5) <= 0.04
    tops, lefts = torch.cat(tops).cpu(), torch.cat(lefts).cpu()
    assert set(tops.tolist()) == set(range(9)) and set(lefts.tolist()) == set(range(5))          # uniform over the valid range: all reached
    s, _ = _stream(gpu, tmp_path, 256, seed=9, augment_horizontal_flip=False)
    assert int(torch.cat([s.draw()[3] for _ in range(4)]).sum()) == 0


def test_stream_sources(gpu, tmp_path):
    from adm_amd.ddm.sr_data import SRBatchStream
    with pytest.raises(NotImplementedError):
        SRBatchStream({"class_name": "ddm.data.EdgeDataset"}, 2, (32, 32), gpu, 1)
    with pytest.raises(ValueError, match="img_folder"):
        SRBatchStream({"class_name": "ddm.data.SRDataset"}, 2, (32, 32), gpu, 1)
    with pytest.raises(NotImplementedError):
        SRBatchStream({"class_name": "synthetic", "inter_type": "lanczos"}, 2, (32, 32), gpu, 1)
    b = next(SRBatchStream({"class_name": "synthetic"}, 2, (32, 32), gpu, 1))          # the synthetic pool runs the same kernel
    assert tuple(b["cond"].shape) == (2, 3, 8, 8) and float(b["image"].min()) >= -1 and float(b["image"].max()) <= 1
    # img_folder: png files of different sizes, found recursively, into the ragged pool
    from PIL import Image
    (tmp_path / "sub").mkdir()
    imgs = {"a.png": R.hash_bytes((40, 36, 3), "sr.f0"), "sub/b.png": R.hash_bytes((33, 50, 3), "sr.f1")}
    for name, a in imgs.items():
        Image.fromarray(a).save(tmp_path / name)
    s = SRBatchStream({"class_name": "ddm.data.SRDataset", "img_folder": str(tmp_path)}, 2, (32, 32), gpu, 1)
    assert s.pool.n == 2 and s.pool.hw.cpu().tolist() == [[40, 36], [33, 50]]
    out = s.next_batch(idx=[1, 0], top=[1, 8], left=[18, 0], flip=[0, 0], want_u8=True)
    pairs = [R.sr_pair(imgs["sub/b.png"], 1, 18, (32, 32)), R.sr_pair(imgs["a.png"], 8, 0, (32, 32))]
    check(out["image"], out["cond"], out["cond_u8"], np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
    with pytest.raises(ValueError, match="smaller than"):
        SRBatchStream({"class_name": "ddm.data.SRDataset", "img_folder": str(tmp_path)}, 2, (36, 36), gpu, 1)


def test_sr_dataset_test_path(gpu, g, tmp_path):
    """SRDatasetTest through sample_cond_ldm.CondStream: the 300x260 golden image -> 512x512 padded frame -> 128x128 condition with
    PIL's bytes; 'image' is the unpadded image; the black padding shows in the last rows."""
    from adm_amd.ddm.sr_data import resample_image
    from sample_cond_ldm import CondStream
    x = g["test.in"]
    np.save(tmp_path / "hr.npy", x[None])
    items = list(CondStream({"class_name": "ddm.data.SRDatasetTest", "npy": str(tmp_path / "hr.npy")}, 1, gpu, seed=1))
    assert len(items) == 1 and items[0]["ori_size"] == (300, 260) and items[0]["img_name"] == f"{0: 010d}.png"
    pad = np.zeros((512, 512, 3), dtype=np.uint8)
    pad[:300, :260] = x
    _, _, u8 = resample_image(pad, 4, "bicubic", gpu, want_u8=True)
    check(items[0]["image"], items[0]["cond"], u8, x[None], g["test.cond"][None])
    assert tuple(items[0]["cond"].shape) == (1, 3, 128, 128)
    assert float(items[0]["cond"][:, :, 80:].max()) == -1.0 and float(items[0]["cond"][:, :, :, 70:].max()) == -1.0
    assert int(g["test.cond"][:74, :64].max()) > 0
