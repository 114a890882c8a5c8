"""GPU: saliency pairs made by adm_pair_resize_batch (adm_amd/csrc/pair_data.hip) against PIL's own bytes
(tests/golden/g23_duts_data.npz) and, for fresh inputs, against tests/duts_data_ref.py (which tests/test_duts_data_host.py pins to
the same golden file).  Everything is compared with torch.equal: the resize is integer arithmetic and the float conversion
(u8 / 255 * 2 - 1, each operation rounded) has one defined order, so there is no tolerance."""
import os

import numpy as np
import pytest
import torch

import duts_data_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_duts_data.npz")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def check(out, want_rgb, want_gray):
    """out = pair_batch(..., want_u8=True); want_rgb uint8 [B,H,W,3], want_gray uint8 [B,H,W]."""
    rgb, gray, rgb_u8, gray_u8 = (t.cpu() for t in out)
    want_rgb, want_gray = torch.from_numpy(np.ascontiguousarray(want_rgb)), torch.from_numpy(np.ascontiguousarray(want_gray))
    print(f"differing bytes: rgb {int((rgb_u8 != want_rgb).sum()) if rgb_u8.shape == want_rgb.shape else 'shape'}, "
          f"gray {int((gray_u8 != want_gray).sum()) if gray_u8.shape == want_gray.shape else 'shape'}")
    assert rgb_u8.dtype == torch.uint8 and gray_u8.dtype == torch.uint8 and rgb.dtype == torch.float32 and gray.dtype == torch.float32
    assert torch.equal(rgb_u8, want_rgb) and torch.equal(gray_u8, want_gray)
    assert torch.equal(rgb, R.to_float(want_rgb.numpy())) and torch.equal(gray, R.gray_to_float(want_gray.numpy()))


def test_golden_cases_in_one_batch(gpu, g):
    """Target 40x56 from 37x53 (up-scaling), 97x131 with an 89x140 map (non-integer down-scale, a map of another size), 40x90 and
    40x56 (identity in one / both axes), 23x200 (up one axis, down the other) and 160x224 (exactly 4x): B = 8, indices 1 and 5
    twice, flips 0 and 1, against PIL's bytes."""
    from adm_amd.ddm.pair_data import PairPool, pair_batch
    assert tuple(g["target"]) == (40, 56)
    draws = g["draws"]
    assert sorted(draws[:, 0].tolist()) == [0, 1, 1, 2, 3, 4, 5, 5] and set(draws[:, 1].tolist()) == {0, 1}
    src = [R.case_sources(i) for i in range(6)]
    assert src[1][0].shape[:2] != src[1][1].shape
    pool = PairPool.from_arrays([p for p, _ in src], [m for _, m in src], (40, 56), gpu)
    out = pair_batch(pool, draws[:, 0], draws[:, 1], want_u8=True)
    sfx = lambda f: "_flipped" if f else ""
    check(out, np.stack([g[f"c{i}.rgb{sfx(f)}"] for i, f in draws]), np.stack([g[f"c{i}.gray{sfx(f)}"] for i, f in draws]))
    # without the uint8 copies the floats are the same
    rgb, gray, a, b = pair_batch(pool, draws[:, 0], draws[:, 1])
    assert a is None and b is None and torch.equal(rgb, out[0]) and torch.equal(gray, out[1])


def test_uint8_intermediate(gpu, g):
    """0 / 255 bytes, 29x45 (map 31x41) -> 16x24: on the CPU a resize that rounds once, after both passes, differs from PIL's bytes
    in both planes, so a kernel without the uint8 intermediate cannot pass."""
    from adm_amd.ddm.pair_data import PairPool, pair_batch
    photo, gmap = g["edge.photo"], g["edge.map"]
    once_rgb = R.resize_rounded_once(photo, (16, 24))
    once_gray = R.resize_rounded_once(np.repeat(gmap[:, :, None], 3, axis=2), (16, 24))[:, :, 0]
    assert int((once_rgb != g["edge.rgb"]).sum()) > 0 and int((once_gray != g["edge.gray"]).sum()) > 0
    pool = PairPool.from_arrays([photo], [gmap], (16, 24), gpu)
    check(pair_batch(pool, [0], [0], want_u8=True), g["edge.rgb"][None], g["edge.gray"][None])


def small_pool(gpu, out=(24, 40)):
    from adm_amd.ddm.pair_data import PairPool
    sizes = [((20, 33), (20, 33)), ((50, 47), (31, 64)), ((24, 70), (24, 70))]
    src = [(R.hash_bytes((ph, pw, 3), f"duts.small.p{i}"), R.hash_bytes((mh, mw), f"duts.small.m{i}"))
           for i, ((ph, pw), (mh, mw)) in enumerate(sizes)]
    return PairPool.from_arrays([p for p, _ in src], [m for _, m in src], out, gpu), src


def test_out_of_range_draws_are_clamped(gpu):
    """idx = N + 3 gives image N - 1's pair, idx = -2 image 0's."""
    from adm_amd.ddm.pair_data import pair_batch
    pool, src = small_pool(gpu)
    want = [R.duts_pair(*src[2], (24, 40)), R.duts_pair(*src[0], (24, 40), flip=True)]
    check(pair_batch(pool, [pool.n + 3, -2], [0, 1], want_u8=True), np.stack([w[0] for w in want]), np.stack([w[1] for w in want]))


def test_over_budget_call_is_refused_without_a_launch(gpu):
    """A call whose declared sources need more LDS than the budget returns ADM_EINVAL and writes nothing."""
    from adm_amd.ddm import pair_data as P
    pool, _ = small_pool(gpu)
    pool.max_h, pool.max_w = 24 * 9, 40 * 9          # what a pool with a 9x source would declare
    pool.kh, pool.kv = P.taps(pool.max_w, 40), P.taps(pool.max_h, 24)
    assert P.lds_need((24, 40), pool.max_h, pool.max_w) > P.LDS_BUDGET
    z = torch.zeros(2, dtype=torch.int32, device=gpu)
    rgb = torch.full((2, 3, 24, 40), 7.5, device=gpu)
    gray = torch.full((2, 1, 24, 40), 7.5, device=gpu)
    rgb_u8 = torch.full((2, 24, 40, 3), 77, dtype=torch.uint8, device=gpu)
    gray_u8 = torch.full((2, 24, 40), 77, dtype=torch.uint8, device=gpu)
    with pytest.raises(RuntimeError, match="adm_pair_resize_batch failed with code -22"):
        P.launch(pool, z, z, rgb, gray, rgb_u8, gray_u8, 2)
    torch.cuda.synchronize()
    assert bool((rgb == 7.5).all()) and bool((gray == 7.5).all()) and bool((rgb_u8 == 77).all()) and bool((gray_u8 == 77).all())


@pytest.fixture(scope="module")
def recipe(gpu):
    """B = 8 at 384x384 from ragged sources between 300 and 420 px (each map of its photo's size but the third): the reference, once."""
    sizes = [(300, 420), (420, 300), (384, 400), (333, 384), (384, 384), (401, 399), (310, 415), (419, 305)]
    src = [(R.hash_bytes((h, w, 3), f"duts.recipe.p{i}"), R.hash_bytes((h - 7, w + 5) if i == 2 else (h, w), f"duts.recipe.m{i}"))
           for i, (h, w) in enumerate(sizes)]
    idx, flip = [3, 0, 7, 2, 5, 1, 6, 4], [0, 1, 1, 0, 0, 1, 0, 1]
    want = [R.duts_pair(*src[i], (384, 384), flip=bool(f)) for i, f in zip(idx, flip)]
    return src, idx, flip, np.stack([w[0] for w in want]), np.stack([w[1] for w in want])


def test_fresh_data_at_the_recipe_shape(gpu, recipe):
    from adm_amd.ddm.pair_data import PairPool, pair_batch
    src, idx, flip, want_rgb, want_gray = recipe
    pool = PairPool.from_arrays([p for p, _ in src], [m for _, m in src], (384, 384), gpu)
    check(pair_batch(pool, idx, flip, want_u8=True), want_rgb, want_gray)


@pytest.mark.parametrize("size,out", [((32, 48), (8, 12)), ((72, 104), (18, 26))])
def test_both_entry_points_are_one_resampler(gpu, size, out):
    """One photo through adm_sr_batch (the crop is the whole image, bilinear) and as the photo of a one-pair pool through
    adm_pair_resize_batch, unflipped and flipped: the same bytes and the same floats, and they are the reference's.  32x48 -> 8x12 is
    the `bilinear` image of tests/golden/g21_sr_data.npz (one tile); 72x104 -> 18x26 crosses tile boundaries in both directions."""
    from adm_amd.ddm.pair_data import PairPool, pair_batch
    from adm_amd.ddm.sr_data import ImagePool, Resampler, sr_batch
    if size == (32, 48):
        sr = np.load(os.path.join(os.path.dirname(GOLDEN), "g21_sr_data.npz"))
        photo, want = sr["bilinear.in"], sr["bilinear.cond"]
        assert str(sr["bilinear.kind"]) == "bilinear" and photo.shape == size + (3,) and want.shape == out + (3,)
    else:
        photo = R.hash_bytes(size + (3,), "duts.one_resampler")
        want = R.resize_rgb(photo, out)
    _, cond, cond_u8 = sr_batch(ImagePool.from_arrays([photo], size, gpu), Resampler(size, out, "bilinear", gpu), [0, 0], [0, 0], [0, 0],
                                [0, 1], want_u8=True)
    pairs = PairPool.from_arrays([photo], [R.hash_bytes(size, "duts.one_resampler.map")], out, gpu)
    rgb, _, rgb_u8, _ = pair_batch(pairs, [0, 0], [0, 1], want_u8=True)
    assert cond_u8.dtype == rgb_u8.dtype == torch.uint8 and cond.dtype == rgb.dtype == torch.float32
    assert torch.equal(cond_u8, rgb_u8) and torch.equal(cond, rgb)
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert torch.equal(rgb_u8[0].cpu(), want) and torch.equal(rgb_u8[1].cpu(), want.flip(1))


def write_tree(root, split_dir, src, tag):
    """png photos under a .jpg name would not decode as the reference's do; real jpgs are lossy, so the tree is READ BACK for the
    expected bytes."""
    from PIL import Image
    img_dir, mask_dir = root / split_dir / f"{split_dir}-Image", root / split_dir / f"{split_dir}-Mask"
    img_dir.mkdir(parents=True), mask_dir.mkdir(parents=True)
    back = []
    for i, (photo, gmap) in enumerate(src):
        name = f"{tag}_{i:03d}"
        Image.fromarray(photo).save(img_dir / f"{name}.jpg", quality=90)
        Image.fromarray(gmap).save(mask_dir / f"{name}.png")
        back.append((np.asarray(Image.open(img_dir / f"{name}.jpg").convert("RGB")), np.asarray(Image.open(mask_dir / f"{name}.png").convert("L"))))
    return back


def test_stream(gpu, tmp_path):
    from adm_amd.ddm.pair_data import DUTSBatchStream
    sizes = [((30, 44), (30, 44)), ((50, 36), (48, 40)), ((33, 33), (33, 33)), ((20, 61), (20, 61)), ((41, 29), (41, 29))]
    mk = lambda tag: [(R.hash_bytes((ph, pw, 3), f"{tag}.p{i}"), R.hash_bytes((mh, mw), f"{tag}.m{i}"))
                      for i, ((ph, pw), (mh, mw)) in enumerate(sizes)]
    tr, te = write_tree(tmp_path, "DUTS-TR", mk("duts.tr"), "tr"), write_tree(tmp_path, "DUTS-TE", mk("duts.te")[:3], "te")
    cfg = {"class_name": "ddm.data.DUTSDataset", "data_root": str(tmp_path), "split": "train", "augment_horizontal_flip": True}
    a, b = DUTSBatchStream(cfg, 2, (32, 40), gpu, 7), DUTSBatchStream(cfg, 2, (32, 40), gpu, 7)
    for _ in range(3):          # the same seed gives the same batches
        ba, bb = next(a), next(b)
        assert list(ba) == ["image", "cond"] and torch.equal(ba["image"], bb["image"]) and torch.equal(ba["cond"], bb["cond"])
    assert tuple(ba["image"].shape) == (2, 1, 32, 40) and tuple(ba["cond"].shape) == (2, 3, 32, 40)
    assert ba["image"].dtype == torch.float32 and float(ba["cond"].min()) >= -1 and float(ba["cond"].max()) <= 1
    # one epoch visits every pair once: two epochs of the 5-pair pool in full batches of 2
    s = DUTSBatchStream(cfg, 2, (32, 40), gpu, 8)
    draws = [s.draw() for _ in range(5)]
    idx = torch.cat([d[0] for d in draws]).cpu()
    assert sorted(idx.tolist()) == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4] and sorted(idx[:5].tolist()) == [0, 1, 2, 3, 4]
    assert idx.dtype == torch.int32 and set(torch.cat([d[1] for d in draws]).cpu().tolist()) <= {0, 1}
    # a drawn batch is what the reference makes of its draws; injected draws are honoured
    i, f = s.draw()
    out = s.next_batch(idx=i, flip=f, want_u8=True)
    want = [R.duts_pair(*tr[int(i[k])], (32, 40), flip=bool(f[k])) for k in range(2)]
    check((out["cond"], out["image"], out["cond_u8"], out["image_u8"]), np.stack([w[0] for w in want]), np.stack([w[1] for w in want]))
    out = s.next_batch(idx=[1, 1], flip=[1, 0], want_u8=True)
    want = [R.duts_pair(*tr[1], (32, 40), flip=True), R.duts_pair(*tr[1], (32, 40))]
    check((out["cond"], out["image"], out["cond_u8"], out["image_u8"]), np.stack([w[0] for w in want]), np.stack([w[1] for w in want]))
    nf = DUTSBatchStream(dict(cfg, augment_horizontal_flip=False), 4, (32, 40), gpu, 9)
    assert int(torch.cat([nf.draw()[1] for _ in range(4)]).sum()) == 0
    # split: test -- DUTS-TE in sorted order, unflipped even when the YAML asks for flips, names and original sizes exposed
    t = DUTSBatchStream(dict(cfg, split="test"), 2, (32, 40), gpu, 7)
    assert t.names == ["te_000.jpg", "te_001.jpg", "te_002.jpg"] and t.ori_sizes == [(30, 44), (50, 36), (33, 33)]
    b1, b2 = t.next_batch(want_u8=True), t.next_batch(want_u8=True)
    assert list(b1)[:2] == ["image", "cond"]
    assert b1["img_name"] == ["te_000.jpg", "te_001.jpg"] and b1["ori_size"] == [(30, 44), (50, 36)]
    assert b2["img_name"] == ["te_002.jpg", "te_000.jpg"] and b2["ori_size"] == [(33, 33), (30, 44)]          # wraps around
    for bt, ids in ((b1, (0, 1)), (b2, (2, 0))):
        want = [R.duts_pair(*te[k], (32, 40)) for k in ids]
        check((bt["cond"], bt["image"], bt["cond_u8"], bt["image_u8"]), np.stack([w[0] for w in want]), np.stack([w[1] for w in want]))


def test_synthetic_stream(gpu):
    from adm_amd.ddm.pair_data import DUTSBatchStream
    cfg = {"class_name": "synthetic", "synthetic_of": "ddm.data.DUTSDataset", "augment_horizontal_flip": True}
    s = DUTSBatchStream(cfg, 4, (48, 64), gpu, 3)
    hw = s.pool.hw_host[0]
    assert (hw[:, 0] < 48).any() and (hw[:, 0] > 48).any() and (hw[:, 1] < 64).any() and (hw[:, 1] > 64).any()
    i, f = s.draw()
    out = s.next_batch(idx=i, flip=f, want_u8=True)
    # the synthetic pool runs the same kernel: its bytes, read back, resize to what the batch holds
    rgb_flat, gray_flat = s.pool.rgb.cpu().numpy(), s.pool.gray.cpu().numpy()
    want = []
    for k in range(4):
        n = int(i[k])
        h, w = (int(v) for v in hw[n])
        ro, go = int(s.pool.rgb_off[n]), int(s.pool.gray_off[n])
        want.append(R.duts_pair(rgb_flat[ro:ro + h * w * 3].reshape(h, w, 3), gray_flat[go:go + h * w].reshape(h, w), (48, 64),
                                flip=bool(f[k])))
    check((out["cond"], out["image"], out["cond_u8"], out["image_u8"]), np.stack([w[0] for w in want]), np.stack([w[1] for w in want]))
