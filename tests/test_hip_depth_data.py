"""GPU: the depth recipe (configs/depth_estimation/) -- adm_depth_batch bit for bit against tests/depth_ref.py and against what PIL
recorded in tests/golden/g29_depth_data.npz, the streams, adm_depth_metrics against float64 NumPy, unet.cond_unet.Unet at the
recipe's map sizes 80 / 40 / 20 / 10 against the CPU oracle, and train_vae.py / train_cond_ldm.py / sample_cond_ldm.py end to end on
reduced YAMLs."""
import importlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import depth_ref as R
from oracle import fill
from oracle import cond_unet_ref as C
from parity import close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = "ddm.data.NYUDv2DepthDataset"


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g29(golden_dir):
    g = np.load(os.path.join(golden_dir, "g29_depth_data.npz"))
    return {"box": tuple(int(v) for v in g["box"]), "photos": [g["photo0"], g["photo1"]], "depths": [g["depth0"], g["depth1"]],
            "cases": g["cases"].tolist(), "out_photo": [g[f"out_photo{k}"] for k in range(len(g["cases"]))],
            "out_depth": [g[f"out_depth{k}"] for k in range(len(g["cases"]))]}


@pytest.fixture(scope="module")
def pool(gpu, g29):
    from adm_amd.ddm.depth_data import DepthPool
    p = DepthPool.from_arrays(g29["photos"], g29["depths"], g29["box"], gpu, ["rgb_0.jpg", "rgb_1.jpg"])
    assert p.n == 2 and p.frame == (19, 24) and [tuple(r) for r in p.hw_host.tolist()] == [(23, 29), (27, 35)]
    assert p.depth_off.tolist() == [0, 2 * 23 * 29] and p.rgb_off.tolist() == [0, 3 * 23 * 29]
    return p


def sentinel_launch(pool, draws, size, margin, image=True, cond=True):
    """adm_depth_batch into the middle of NaN-filled buffers, `margin` floats from either end: (image, cond) and the margins checked."""
    from adm_amd.ddm import depth_data as D
    dev = pool.depth.device
    idx, top, left, flip = (torch.tensor(v, dtype=torch.int32, device=dev) for v in draws)
    B, (H, W) = len(draws[0]), size
    outs = []
    for want, ch in ((image, 1), (cond, 3)):
        if not want:
            outs.append((None, None))
            continue
        buf = torch.full((2 * margin + B * ch * H * W,), float("nan"), device=dev, dtype=torch.float32)
        outs.append((buf, buf[margin:margin + B * ch * H * W].view(B, ch, H, W)))
    D.launch(pool, idx, top, left, flip, outs[0][1], outs[1][1], B, H, W)
    torch.cuda.synchronize()
    for buf, view in outs:
        if buf is not None:
            assert bool(torch.isnan(buf[:margin]).all()) and bool(torch.isnan(buf[-margin:]).all()), "a store outside the output"
            assert not bool(torch.isnan(view).any())
    return outs[0][1], outs[1][1]


@pytest.mark.parametrize("size,margin", [((16, 20), 8), ((16, 20), 3), ((15, 18), 8), ((15, 18), 5)])
def test_batch_equals_numpy_and_pil_bit_for_bit(gpu, g29, pool, size, margin):
    """One launch per output size over all of g29's draws of that size: offsets at 0 and at their maxima, odd lefts (depth rows
    2-byte aligned only, photo rows at any byte), flips 0 and 1 in one batch, a repeated pair, depths 0 / 1 / 9999 / 10000 / 65535.
    Width 20 with a 16-byte aligned output takes the 16-byte stores, with the output 12 bytes off the scalar form; width 18 is no
    multiple of 4."""
    ks = [k for k, c in enumerate(g29["cases"]) if (c[4], c[5]) == size and not c[6]]
    assert len(ks) == 5
    draws = [[g29["cases"][k][j] for k in ks] for j in range(4)]
    assert {0, 1} == set(draws[3]) and len(set(draws[0])) < len(draws[0]) and any(l % 2 for l in draws[2]) and 0 in draws[1]
    image, cond = sentinel_launch(pool, draws, size, margin)
    want_i, want_c = R.batch(g29["photos"], g29["depths"], g29["box"], *draws, size)
    assert torch.equal(image.cpu(), torch.from_numpy(want_i)) and torch.equal(cond.cpu(), torch.from_numpy(want_c))
    pil_i = np.stack([R.depth_to_float(g29["out_depth"][k])[None] for k in ks])
    pil_c = np.stack([R.photo_to_float(g29["out_photo"][k]) for k in ks])
    assert torch.equal(image.cpu(), torch.from_numpy(pil_i)) and torch.equal(cond.cpu(), torch.from_numpy(pil_c))
    if size == (16, 20):
        assert float(image.max()) == float(np.float32(65535) / np.float32(10000) * np.float32(2) - np.float32(1)) and float(image.min()) == -1.0
    # either output alone: the same values, and the other pool is not needed
    only_i, none = sentinel_launch(pool, draws, size, margin, cond=False)
    assert none is None and torch.equal(only_i, image)
    none, only_c = sentinel_launch(pool, draws, size, margin, image=False)
    assert none is None and torch.equal(only_c, cond)


def test_whole_frame_form_and_the_wrapper(gpu, g29, pool):
    """The test item: top = left = 0, the boxed frame's own size, no flip, B = 1 -- against PIL's ``.crop(box)`` alone."""
    from adm_amd.ddm import depth_data as D
    for k, c in enumerate(g29["cases"]):
        if not c[6]:
            continue
        image, cond = D.depth_batch(pool, [c[0]], [0], [0], [0], pool.frame)
        assert tuple(image.shape) == (1, 1, 19, 24) and tuple(cond.shape) == (1, 3, 19, 24)
        assert torch.equal(image.cpu()[0, 0], torch.from_numpy(R.depth_to_float(g29["out_depth"][k])))
        assert torch.equal(cond.cpu()[0], torch.from_numpy(R.photo_to_float(g29["out_photo"][k])))
    # out-of-range draws are clamped, not followed
    a = D.depth_batch(pool, [7, -3], [99, -5], [99, -5], [0, 0], (16, 20))
    b = D.depth_batch(pool, [1, 0], [3, 0], [4, 0], [0, 0], (16, 20))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match="a 20x24 crop does not fit the 19x24 frame"):
        D.depth_batch(pool, [0], [0], [0], [0], (20, 24))
    with pytest.raises(ValueError, match="a draw has 1 entries, the batch 2"):
        D.depth_batch(pool, [0, 1], [0], [0, 0], [0, 0], (16, 20))
    # a pool of depth maps only makes the depth plane, and says so when asked for more
    alone = D.DepthPool.from_arrays(None, g29["depths"], g29["box"], gpu)
    assert alone.rgb is None and alone.nbytes == alone.depth.numel()
    img, none = D.depth_batch(alone, [1, 0], [3, 0], [4, 0], [1, 0], (16, 20), cond=False)
    assert none is None and torch.equal(img, D.depth_batch(pool, [1, 0], [3, 0], [4, 0], [1, 0], (16, 20))[0])
    with pytest.raises(ValueError, match="holds no photos"):
        D.depth_batch(alone, [0], [0], [0], [0], (16, 20))
    # the C ABI refuses what it cannot address
    z = torch.zeros(1, dtype=torch.int32, device=gpu)
    out = torch.empty(1, 1, 16, 20, device=gpu)
    args = lambda box, H=16, W=20: (None, 0, None, None, D.ptr(alone.depth), alone.depth.numel(), D.ptr(alone.depth_off),
                                    D.ptr(alone.depth_hw), alone.n, *box, D.ptr(z), D.ptr(z), D.ptr(z), D.ptr(z), D.ptr(out), None, 1, H, W)
    for bad in (args((3, 2, 22, 21)), args((-1, 2, 27, 21)), args(g29["box"], 0, 20)):
        with pytest.raises(RuntimeError, match="adm_depth_batch failed with code -22"):
            D.call("adm_depth_batch", *bad)
    with pytest.raises(RuntimeError, match="code -22"):
        D.call("adm_depth_batch", *args(g29["box"])[:17], None, None, 1, 16, 20)          # neither output


def pool_arrays(p):
    """The pool read back to the host as (photos uint8 [h,w,3], depths uint16 [h,w])."""
    d = p.depth.cpu().numpy().view("<u2")
    rgb = p.rgb.cpu().numpy() if p.rgb is not None else None
    photos, depths = [], []
    for i, (h, w) in enumerate(p.hw_host.tolist()):
        o = int(p.depth_off[i]) // 2
        depths.append(d[o:o + h * w].reshape(h, w).astype(np.uint16))
        if rgb is not None:
            o = int(p.rgb_off[i])
            photos.append(rgb[o:o + 3 * h * w].reshape(h, w, 3))
    return photos, depths


CFG = {"class_name": "synthetic", "synthetic_of": FULL, "border_crop": [3, 2, 35, 28], "augment_horizontal_flip": True}


def test_stream_draws_batches_and_epochs(gpu):
    from adm_amd.ddm.depth_data import DepthBatchStream
    s = DepthBatchStream(CFG, 5, (16, 20), gpu, seed=3)
    n = s.pool.n
    assert n == 12 and s.pool.frame == (26, 32) and sorted(set(map(tuple, s.pool.hw_host.tolist()))) == [(28, 35), (37, 74), (52, 51)]
    photos, depths = pool_arrays(s.pool)
    assert all(int(d.max()) <= 10000 for d in depths) and max(int(d.max()) for d in depths) > 9900
    twin = DepthBatchStream(CFG, 5, (16, 20), gpu, seed=3)
    other = DepthBatchStream(CFG, 5, (16, 20), gpu, seed=4)
    seen, flips, differs = [], [], False
    for step in range(6):          # 30 draws of 12 pairs: two epoch boundaries inside batches
        idx, top, left, flip = (t.cpu().tolist() for t in s.draw())
        assert len(idx) == 5 and all(0 <= i < n for i in idx) and all(0 <= t <= 10 for t in top) and all(0 <= l <= 12 for l in left)
        assert set(flip) <= {0, 1}
        seen += idx
        flips += flip
        batch = s.next_batch(idx=idx, top=top, left=left, flip=flip)
        assert list(batch) == ["image", "cond"] and tuple(batch["image"].shape) == (5, 1, 16, 20) and tuple(batch["cond"].shape) == (5, 3, 16, 20)
        want_i, want_c = R.batch(photos, depths, s.box, idx, top, left, flip, (16, 20))
        assert torch.equal(batch["image"].cpu(), torch.from_numpy(want_i)) and torch.equal(batch["cond"].cpu(), torch.from_numpy(want_c))
        # the same seed gives the same batches; the twin draws for itself (next() consumes what draw() + next_batch(...) did)
        again = next(twin)
        assert torch.equal(again["image"], batch["image"]) and torch.equal(again["cond"], batch["cond"])
        differs |= not torch.equal(next(other)["image"], batch["image"])
    assert differs
    assert sorted(seen[:12]) == sorted(seen[12:24]) == list(range(12)) and set(flips) == {0, 1}
    assert len(set(map(tuple, [seen[:12], seen[12:24]]))) == 2          # a fresh permutation per epoch
    # one flip draw for both planes: the flipped batch is the mirrored batch
    a = s.next_batch(idx=[4, 5], top=[3, 10], left=[1, 12], flip=[0, 0])
    b = s.next_batch(idx=[4, 5], top=[3, 10], left=[1, 12], flip=[1, 1])
    assert torch.equal(b["image"], a["image"].flip(-1)) and torch.equal(b["cond"], a["cond"].flip(-1))
    # without augment_horizontal_flip no flip is drawn
    plain = DepthBatchStream(dict(CFG, augment_horizontal_flip=False), 5, (16, 20), gpu, seed=3)
    assert all(int(plain.draw()[3].sum()) == 0 for _ in range(3))


def test_test_split_and_the_first_stage_stream(gpu, tmp_path):
    from adm_amd.ddm.depth_data import DepthBatchStream, DepthMapStream
    s = DepthBatchStream(dict(CFG, split="test"), 1, (16, 20), gpu, seed=0)
    photos, depths = pool_arrays(s.pool)
    for i in (0, 1, 2):
        item = next(s)
        assert item["img_name"] == [f"rgb_{i:05d}.jpg"] and item["ori_size"] == [(26, 32)]
        want_i, want_c = R.batch(photos, depths, s.box, [i], [0], [0], [0], (26, 32))
        assert torch.equal(item["image"].cpu(), torch.from_numpy(want_i)) and torch.equal(item["cond"].cpu(), torch.from_numpy(want_c))
    item = s.next_batch(idx=[7], flip=[0])          # as sample_cond_ldm.DatasetCondStream asks
    assert item["img_name"] == ["rgb_00007.jpg"] and tuple(item["cond"].shape) == (1, 3, 26, 32)
    m = DepthMapStream(CFG, 4, (16, 20), gpu, seed=3)
    assert m.channels == 1 and m.pool.rgb is None
    batch = next(m)
    assert list(batch) == ["image"] and tuple(batch["image"].shape) == (4, 1, 16, 20)
    draws = dict(idx=[3, 3, 11, 0], top=[0, 10, 5, 1], left=[12, 0, 7, 3], flip=[1, 0, 1, 0])
    both = DepthBatchStream(CFG, 4, (16, 20), gpu, seed=3)          # the same seed: the depth planes are drawn first, so they agree
    assert torch.equal(m.next_batch(**draws)["image"], both.next_batch(**draws)["image"])
    # real files: train/ has two 30x40 pairs, 'full' all three; the photos are never opened by the first-stage stream
    R.nyud_tree(tmp_path)
    real = dict(CFG, class_name=FULL, data_root=str(tmp_path), split="full", border_crop=[3, 2, 35, 28])
    s = DepthBatchStream(real, 2, (16, 20), gpu, seed=1)
    assert s.pool.n == 3 and s.names == ["rgb_00002.jpg", "rgb_00000.jpg", "rgb_00001.jpg"] and s.pool.box == (0, 0, 32, 26)
    got = s.next_batch(idx=[1, 0], top=[10, 0], left=[12, 5], flip=[1, 0])
    d0 = R.hash_values((30, 40), "tree.d0", 10001).astype(np.uint16)
    d2 = R.hash_values((33, 41), "tree.d2", 10001).astype(np.uint16)
    want = np.stack([R.depth_to_float(R.crop(d0, (3, 2, 35, 28), 10, 12, (16, 20), 1))[None],
                     R.depth_to_float(R.crop(d2, (3, 2, 35, 28), 0, 5, (16, 20), 0))[None]])
    assert torch.equal(got["image"].cpu(), torch.from_numpy(want))
    for p in tmp_path.rglob("*.jpg"):
        p.write_bytes(b"never opened")
    m = DepthMapStream(dict(real, split="train"), 2, (16, 20), gpu, seed=1)
    assert m.pool.n == 2 and m.pool.rgb is None and tuple(next(m)["image"].shape) == (2, 1, 16, 20)


def metric_case(shape, seed):
    """g ~ U(0.5, 9.5) m, p = g exp(N(0, 0.25)); image 0 (of several) wholly invalid; zeros and max_depth in the gt; predictions outside
    [min, max]."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.05, 0.95, shape)
    p = g * np.exp(rng.normal(0.0, 0.25, shape))
    g, p = g.astype(np.float32), p.astype(np.float32)
    flat_g, flat_p = g.reshape(shape[0], -1), p.reshape(shape[0], -1)
    flat_g[-1, 0:3] = 0.0          # invalid: zero
    flat_g[-1, 3:5] = 1.0          # invalid: exactly max_depth
    flat_p[-1, 5] = 1.7            # clamped to max_depth
    flat_p[-1, 6] = 0.0            # clamped to min_depth
    flat_p[-1, 7] = -0.3
    if shape[0] > 1:
        flat_g[0, :] = 0.0
        flat_g[0, ::2] = 1.0
    return p, g


@pytest.mark.parametrize("shape", [(1, 1, 7, 9), (3, 1, 33, 41)])
def test_metrics_against_float64_numpy(gpu, shape):
    from adm_amd.metrics import depth as M
    p, g = metric_case(shape, 11 + shape[0])
    r = R.ratios(p, g)
    margin = min(float(np.abs(r - t).min()) for t in R.THRESHOLDS)
    print(f"{shape}: {r.size} valid pixels, closest ratio to a 1.25^k threshold: {margin:.3e}; below: "
          + ", ".join(f"{float((r < t).mean()):.3f}" for t in R.THRESHOLDS))
    assert margin > 1e-9          # so the three counts do not depend on the last bit of a division
    want = R.sums(p, g)
    assert all(0 < want[-1, 7 + k] < want[-1, 0] for k in range(3)) and want[-1, 7] < want[-1, 8] < want[-1, 9]
    pd, gd = torch.from_numpy(p).to(gpu), torch.from_numpy(g).to(gpu)
    got = M.depth_sums(pd, gd)
    assert got.dtype == torch.float64 and tuple(got.shape) == (shape[0], 10)
    again = M.depth_sums(pd, gd)
    assert torch.equal(got, again)          # identical bits
    got = got.cpu().numpy()
    assert np.array_equal(got[:, [0, 7, 8, 9]], want[:, [0, 7, 8, 9]])
    rel = np.abs(got[:, 1:7] - want[:, 1:7]) / np.maximum(np.abs(want[:, 1:7]), 1e-300)
    print("relative error of the six sums:", rel.max(axis=0))
    assert float(rel[want[:, 0] > 0].max()) <= 1e-10 and np.all(got[want[:, 0] == 0] == 0)
    res, ref = M.metrics_from_sums(got), R.metrics(want)
    assert res["skipped"] == ref["skipped"] == (1 if shape[0] > 1 else 0) and res["images"] == shape[0] - res["skipped"]
    for k in M.KEYS:
        assert res[k] == pytest.approx(ref[k], rel=1e-9), k
    score = M.DepthScore()
    score.add(pd, gd)
    score.add(pd[-1:], gd[-1:])
    both = score.result()
    assert both["images"] == res["images"] + 1 and both["skipped"] == res["skipped"]
    with pytest.raises(ValueError, match=r"must both be \[B,1,H,W\]"):
        M.depth_sums(pd[:, 0], gd[:, 0])


@pytest.mark.parametrize("shape,blocks", [((2, 1, 426, 560), 59), ((1, 1, 520, 520), 64)])
def test_metrics_with_many_partials(gpu, shape, blocks):
    """The recipe's frame, 426x560: 59 workgroups per image; 520x520 is past 64 chunks of 4096, so the chunks grow instead.  The last
    workgroup adds the partials in order -- equal counts, the sums to 1e-10 (N <= 270400 terms of a few ulp: under 1e-10), the same
    bits on every one of five runs."""
    from adm_amd import hip
    from adm_amd.metrics import depth as M
    assert hip.lib().adm_depth_metrics_blocks(shape[2] * shape[3]) == blocks
    p, g = metric_case(shape, 5)
    want = R.sums(p, g)
    pd, gd = torch.from_numpy(p).to(gpu), torch.from_numpy(g).to(gpu)
    runs = [M.depth_sums(pd, gd) for _ in range(5)]
    assert all(torch.equal(runs[0], r) for r in runs[1:])
    got = runs[0].cpu().numpy()
    assert np.array_equal(got[:, 0], want[:, 0]) and got[-1, 0] == shape[2] * shape[3] - 5 and (shape[0] == 1 or got[0, 0] == 0)
    ratios = R.ratios(p, g)
    assert min(float(np.abs(ratios - t).min()) for t in R.THRESHOLDS) > 1e-9
    assert np.array_equal(got[:, 7:], want[:, 7:])
    assert float((np.abs(got[-1, 1:7] - want[-1, 1:7]) / np.abs(want[-1, 1:7])).max()) <= 1e-10


def test_eval_depth_scores_a_folder(gpu, tmp_path, capsys):
    """eval_depth.py on a small tree: boxed and whole-frame predictions, the JSON against tests/depth_ref.py; a missing prediction
    and one of a third size are named."""
    import eval_depth
    from adm_amd.ddm.depth_data import write_depth_png
    R.nyud_tree(tmp_path / "nyud")
    box = (3, 2, 35, 28)
    pred_dir = tmp_path / "pred"
    pred_dir.mkdir()
    preds, gts = [], []
    for i, (h, w) in ((0, (30, 40)), (1, (30, 40))):
        gt = R.hash_values((h, w), f"tree.d{i}", 10001).astype(np.uint16)
        pred = np.clip(gt.astype(np.int64) + R.hash_values((h, w), f"eval.p{i}", 2001) - 1000, 0, 65535).astype(np.uint16)
        write_depth_png(pred_dir / f"rgb_{i:05d}.png", pred if i else np.ascontiguousarray(pred[2:28, 3:35]))          # boxed, then whole
        preds.append(pred[2:28, 3:35].astype(np.float32) / np.float32(10000))
        gts.append(gt[2:28, 3:35].astype(np.float32) / np.float32(10000))
    argv = ["--pred", str(pred_dir), "--data_root", str(tmp_path / "nyud"), "--split", "train", "--border_crop", *map(str, box),
            "--out_path", str(tmp_path / "result.json")]
    res = eval_depth.main(argv)
    want = R.metrics(R.sums(np.stack(preds)[:, None], np.stack(gts)[:, None]))
    assert res["images"] == 2 and res["skipped"] == 0 and json.load(open(tmp_path / "result.json")) == res
    for k in R.KEYS:
        assert res[k] == pytest.approx(want[k], rel=1e-9), k
    write_depth_png(pred_dir / "rgb_00001.png", np.zeros((26, 33), np.uint16))
    with pytest.raises(ValueError, match="rgb_00001.png is 26x33: expected the boxed frame 26x32 or the whole frame 30x40"):
        eval_depth.main(argv)
    (pred_dir / "rgb_00000.png").unlink()
    with pytest.raises(FileNotFoundError, match="the prediction for .*rgb_00000.jpg is missing"):
        eval_depth.main(argv)


def test_denoiser_at_the_recipe_map_sizes_vs_oracle(gpu):
    """unet.cond_unet.Unet with dim 32 x (1, 2, 4, 4), windows 8 / 4 / 2 / 1 on both sides, an 80x80 latent (maps 80 / 40 / 20 / 10:
    the recipe's own, 320 / 4), B = 1, the four condition maps given directly: forward, the gradients of every input and of the
    weights against the CPU oracle, at the bars tests/test_hip_saliency.py holds the same model to at 48 / 24 / 12."""
    wins = [[8, 8], [4, 4], [2, 2], [1, 1]]
    cfg = C.default_cfg(dim=32, two_decoders=True, window_sizes1=wins, window_sizes2=wins)
    mod = importlib.import_module("unet.cond_unet")
    m = mod.Unet(dim=32, dim_mults=cfg["dim_mults"], cond_dim=32, cond_dim_mults=(), channels=3, cond_in_dim=3, window_sizes1=wins,
                 window_sizes2=wins, fourier_scale=16, cfg={"cond_net": "swin", "cond_pe": False})
    sd = C.filled_state_dict(cfg)
    m.load_state_dict(sd, strict=True)
    for mm in m.modules():
        if isinstance(mm, torch.nn.Dropout):
            mm.p = 0.0
    m = m.to(gpu).eval()
    x = fill.hash_tensor((1, 3, 80, 80), "dep.x", 1.0)
    tt = torch.tensor([0.4])
    hm = C.cond_features(1, 320, 320, tag="dep.hm")
    assert [tuple(h.shape[2:]) for h in hm] == [(80, 80), (40, 40), (20, 20), (10, 10)]
    gx, gy = fill.hash_tensor((1, 3, 80, 80), "dep.gx", 1.0), fill.hash_tensor((1, 3, 80, 80), "dep.gy", 1.0)
    xg = x.to(gpu).requires_grad_(True)
    hg = [h.to(gpu).requires_grad_(True) for h in hm]
    y1, y2 = m(xg, tt.to(gpu), hg)
    sdo = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k and k != "time_mlp.0.W" else v.clone())
           for k, v in sd.items()}
    xo, ho = x.clone().requires_grad_(True), [h.clone().requires_grad_(True) for h in hm]
    o1, o2 = C.unet_forward(sdo, cfg, xo, tt, ho)
    close(y1, o1.detach()); close(y2, o2.detach())
    ((y1 * gx.to(gpu)).sum() + (y2 * gy.to(gpu)).sum()).backward()
    ((o1 * gx).sum() + (o2 * gy).sum()).backward()
    close(xg.grad, xo.grad)
    for got, want in zip(hg, ho):
        close(got.grad, want.grad)
    gmax = max(float(v.grad.double().norm()) for v in sdo.values() if v.requires_grad and v.grad is not None)
    named = {n: p for n, p in m.named_parameters() if p.requires_grad}
    bad = []
    for name, p in named.items():
        want = sdo[name].grad
        err = float((p.grad.cpu().double() - want.double()).norm() / (want.double().norm() + 1e-4 * gmax))
        if err > 2e-3:
            bad.append((name, err))
    assert not bad, bad[:10]
    names = list(named)
    for name in (names[0], names[len(names) // 4], names[len(names) // 2], names[3 * len(names) // 4], names[-1]):
        want = sdo[name].grad
        close(named[name].grad, want, scale=max(float(want.double().norm()) / 8, 1e-12))


BOX = [3, 2, 99, 82]          # an 80 x 96 frame: larger than the 64x64 model, so training crops and sampling slides


def run(script, path, *extra):
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, script), "--cfg", path, *extra],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def reduced(name, tmp_path):
    cfg = yaml.load(open(os.path.join(ROOT, "configs", "depth_estimation", name)), Loader=yaml.SafeLoader)
    assert cfg["data"]["class_name"] == "synthetic" and cfg["data"]["synthetic_of"] == FULL
    cfg["data"].update(image_size=[64, 64], batch_size=2, border_crop=BOX)
    return cfg, str(tmp_path / "run")


def test_first_stage_cli_trains_on_depth_planes(gpu, tmp_path):
    cfg, res = reduced("nyud_ae_kl_320x320.yaml", tmp_path)
    assert cfg["data"]["split"] == "full" and cfg["model"]["ddconfig"]["in_channels"] == 1
    cfg["model"]["ddconfig"].update(ch=32, resolution=[64, 64])
    cfg["trainer"].update(results_folder=res, train_num_steps=2, save_and_sample_every=2, log_freq=1, ema_update_after_step=1,
                          ema_update_every=1)
    path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    out = run("train_vae.py", path, "--max-steps", "2")
    assert "depth map pool: 12 pairs (depth planes only), frames of 80x96 inside the border box" in out
    steps = re.findall(r"\[Train Step\] (\d+)/2: .*nll_loss=(\S+)", out)
    assert [int(s) for s, _ in steps] == [0, 1] and all(np.isfinite(float(v)) and float(v) > 0 for _, v in steps), out[-2000:]
    ck = torch.load(os.path.join(res, "model-1.pt"), map_location="cpu", weights_only=True)
    assert ck["step"] == 2 and tuple(ck["model"]["encoder.conv_in.weight"].shape) == (32, 1, 3, 3)


def test_train_and_sample_depth_cli_end_to_end(gpu, tmp_path):
    from PIL import Image
    cfg, res = reduced("nyud_cond_ddm_const_ldm.yaml", tmp_path)
    cfg["model"].update(image_size=[64, 64], sampling_timesteps=2)
    cfg["model"]["first_stage"]["ddconfig"].update(ch=32, resolution=[64, 64])
    cfg["model"]["unet"].update(dim=32, cond_feature_size=[16, 16])
    cfg["trainer"].update(results_folder=res, gradient_accumulate_every=2, train_num_steps=2, save_and_sample_every=2, log_freq=1,
                          test_before=False, ema_update_after_step=1, ema_update_every=1, resume_milestone=0)
    path = str(tmp_path / "train.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    out = run("train_cond_ldm.py", path, "--max-steps", "2")
    assert "depth pool: 12 pairs (photo + depth planes), frames of 80x96 inside the border box" in out
    losses = [float(v) for v in re.findall(r"\[Train Step\] \d+/2: loss=(\S+)", out)]
    assert len(losses) == 2 and all(np.isfinite(losses)), out[-2000:]
    assert torch.load(os.path.join(res, "model-1.pt"), map_location="cpu", weights_only=True)["step"] == 2
    # the sampler: whole 80x96 frames in 2 x 2 windows of 64x64 at stride 32, each twice (flip_test), 16-bit files and the score
    sample, _ = reduced("nyud_cond_ddm_const_ldm_sample.yaml", tmp_path)
    assert sample["data"]["split"] == "test" and sample["sampler"]["flip_test"] is True
    sample["model"] = cfg["model"]
    png = os.path.join(res, "png")
    sample["sampler"].update(sample_num=2, crop_size=[64, 64], stride=[32, 32], save_folder=png)
    path = str(tmp_path / "sample.yaml")
    yaml.safe_dump(sample, open(path, "w"))
    out = run("sample_cond_ldm.py", path, "--random-init", "--max-images", "2")
    assert "depth score over 2 images (0 without a valid pixel)" in out and "PSNR" not in out
    assert sorted(os.listdir(png)) == ["depth_metrics.json", "rgb_00000.png", "rgb_00001.png"]
    for n in ("rgb_00000.png", "rgb_00001.png"):
        im = Image.open(os.path.join(png, n))
        assert im.mode == "I;16" and im.size == (96, 80), (n, im.mode, im.size)
        assert int(np.array(im).max()) <= 10000
    res_json = json.load(open(os.path.join(png, "depth_metrics.json")))
    assert set(res_json) == {"abs_rel", "sq_rel", "rmse", "rmse_log", "silog", "log10", "d1", "d2", "d3", "images", "skipped"}
    assert all(np.isfinite(res_json[k]) for k in res_json) and res_json["images"] == 2 and 0 <= res_json["d1"] <= res_json["d3"] <= 1
    # the reference's 8-bit files stay available
    sample["sampler"].update(depth_png8=True, save_folder=png + "8")
    yaml.safe_dump(sample, open(path, "w"))
    run("sample_cond_ldm.py", path, "--random-init", "--max-images", "1")
    im = Image.open(os.path.join(png + "8", "rgb_00000.png"))
    assert im.mode == "L" and im.size == (96, 80)
