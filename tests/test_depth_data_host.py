"""Host: the depth recipe's data path without a device -- tests/depth_ref.py against what PIL recorded in
tests/golden/g29_depth_data.npz, the file discovery, every refusal with its message, the dataset table, the C ABI's two entry points,
the 16-bit png and the metric definitions."""
import os
import re

import numpy as np
import pytest
import torch

import depth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL, SHORT = "ddm.data.NYUDv2DepthDataset", "NYUDv2DepthDataset"


@pytest.fixture(scope="module")
def g29(golden_dir):
    return np.load(os.path.join(golden_dir, "g29_depth_data.npz"))


def test_depth_ref_equals_pil_bit_for_bit(g29):
    box = tuple(int(v) for v in g29["box"])
    photos, depths = [g29["photo0"], g29["photo1"]], [g29["depth0"], g29["depth1"]]
    assert depths[0].dtype == np.uint16 and photos[0].dtype == np.uint8
    cases = g29["cases"]
    assert len(cases) == 12 and {int(c[5]) % 4 for c in cases} == {0, 2} and {int(c[3]) for c in cases} == {0, 1}
    seen = set()
    for k, (i, top, left, flip, H, W, whole) in enumerate(cases.tolist()):
        if whole:
            assert (H, W) == (box[3] - box[1], box[2] - box[0])
        got_d = R.crop(depths[i], box, top, left, (H, W), flip)
        got_p = R.crop(photos[i], box, top, left, (H, W), flip)
        assert got_d.dtype == np.uint16 and np.array_equal(got_d, g29[f"out_depth{k}"]), k
        assert np.array_equal(got_p, g29[f"out_photo{k}"]), k
        seen |= set(np.unique(got_d).tolist())
        image, cond = R.batch(photos, depths, box, [i], [top], [left], [flip], (H, W))
        assert image.dtype == np.float32 and image.shape == (1, 1, H, W) and cond.shape == (1, 3, H, W)
        # the float maps of PIL's own arrays, the reference's operations (data.py:879-886) in torch
        want = torch.from_numpy(g29[f"out_depth{k}"].astype(np.float32)) / 10000 * 2 - 1
        assert torch.equal(torch.from_numpy(image[0, 0]), want), k
        wantc = (torch.from_numpy(g29[f"out_photo{k}"]).permute(2, 0, 1).to(torch.float32) / 255) * 2 - 1
        assert torch.equal(torch.from_numpy(cond[0]), wantc), k
    assert {0, 1, 9999, 10000, 65535} <= seen
    assert float(R.depth_to_float(np.asarray([65535], dtype=np.uint16))[0]) == pytest.approx(12.107, abs=1e-6)          # no clipping


def test_find_nyud_pairs_by_split(tmp_path):
    from adm_amd.ddm.depth_data import find_nyud_pairs, load_nyud
    R.nyud_tree(tmp_path)
    names = lambda split: [(p.name, d.name) for p, d in find_nyud_pairs(str(tmp_path), split)]
    assert names("train") == [("rgb_00000.jpg", "sync_depth_00000.png"), ("rgb_00001.jpg", "sync_depth_00001.png")]
    assert names("test") == [("rgb_00002.jpg", "sync_depth_00002.png")]
    assert [n for n, _ in names("full")] == ["rgb_00002.jpg", "rgb_00000.jpg", "rgb_00001.jpg"]          # sorted by path: test/ < train/
    assert all(p.parent == d.parent for p, d in find_nyud_pairs(str(tmp_path), "full"))
    with pytest.raises(FileNotFoundError, match="no jpg photo below"):
        find_nyud_pairs(str(tmp_path / "test" / "bathroom" / "nothing"), "full")
    # only the boxed region is kept, and without photos no photo is opened
    box = (3, 2, 35, 28)
    photos, depths, kept = load_nyud(str(tmp_path), "full", box)
    assert kept == ["rgb_00002.jpg", "rgb_00000.jpg", "rgb_00001.jpg"]
    assert all(p.shape == (26, 32, 3) and p.dtype == np.uint8 for p in photos) and all(d.shape == (26, 32) and d.dtype == np.uint16 for d in depths)
    assert np.array_equal(depths[1], R.hash_values((30, 40), "tree.d0", 10001).astype(np.uint16)[2:28, 3:35])
    (tmp_path / "test" / "bathroom" / "rgb_00002.jpg").write_bytes(b"not a jpg")
    photos, depths, _ = load_nyud(str(tmp_path), "test", box, photos=False)
    assert photos is None and len(depths) == 1
    with pytest.raises(OSError, match="rgb_00002.jpg cannot be read"):
        load_nyud(str(tmp_path), "test", box)


def test_refusals_name_the_file(tmp_path):
    from adm_amd.ddm.depth_data import DepthBatchStream, DepthPool, find_nyud_pairs, load_nyud
    R.nyud_tree(tmp_path)
    # a frame smaller than the box: the 30x40 frames do not hold a box that needs 31 rows; the 33x41 one does
    with pytest.raises(ValueError, match=r"pair 0 \(rgb_00000.jpg\): the frame is 30x40, smaller than the border box \(3, 2, 35, 31\)"):
        load_nyud(str(tmp_path), "train", (3, 2, 35, 31))
    assert len(load_nyud(str(tmp_path), "test", (3, 2, 35, 31))[1]) == 1
    # a missing depth file
    missing = tmp_path / "train" / "office_0002" / "sync_depth_00001.png"
    missing.unlink()
    with pytest.raises(FileNotFoundError, match=re.escape(f"the depth map of {tmp_path / 'train' / 'office_0002' / 'rgb_00001.jpg'} is missing: {missing}")):
        find_nyud_pairs(str(tmp_path), "train")
    # the planes of a pair disagree
    photos = [np.zeros((30, 40, 3), np.uint8), np.zeros((30, 40, 3), np.uint8)]
    depths = [np.zeros((30, 40), np.uint16), np.zeros((30, 41), np.uint16)]
    with pytest.raises(ValueError, match=r"pair 1 \(b.jpg\): its photo is 30x40 but its depth map is 30x41"):
        DepthPool.from_arrays(photos, depths, (0, 0, 40, 30), "cpu", ["a.jpg", "b.jpg"])
    with pytest.raises(ValueError, match="2 photos but 1 depth maps"):
        DepthPool.from_arrays(photos, depths[:1], (0, 0, 40, 30), "cpu")
    with pytest.raises(ValueError, match="expected a non-empty uint16"):
        DepthPool.from_arrays(photos[:1], [np.zeros((30, 40), np.uint8)], (0, 0, 40, 30), "cpu")
    # a crop larger than the boxed frame, as T.RandomCrop
    cfg = {"class_name": "synthetic", "synthetic_of": FULL, "border_crop": [3, 2, 35, 28]}
    with pytest.raises(ValueError, match=r"image_size 27x32 is larger than the 26x32 frame data.border_crop \[3, 2, 35, 28\] leaves"):
        DepthBatchStream(cfg, 2, (27, 32), "cpu", 0)
    with pytest.raises(ValueError, match="image_size 320x561 is larger than the 426x560 frame"):
        DepthBatchStream({"class_name": "synthetic", "synthetic_of": FULL}, 2, (320, 561), "cpu", 0)
    with pytest.raises(ValueError, match="border_crop"):
        DepthBatchStream(dict(cfg, border_crop=[3, 2, 3, 28]), 2, (8, 8), "cpu", 0)
    with pytest.raises(NotImplementedError, match="only ddm.data.NYUDv2DepthDataset \\+ data_root, or 'synthetic'"):
        DepthBatchStream({"class_name": "ddm.data.NYUDv2DepthDataset2", "data_root": str(tmp_path)}, 2, (8, 8), "cpu", 0)
    with pytest.raises(ValueError, match="needs data.data_root"):
        DepthBatchStream({"class_name": FULL}, 2, (8, 8), "cpu", 0)


def test_the_table_selects_the_depth_streams(monkeypatch):
    import sample_cond_dpm
    import sample_cond_ldm
    import train_cond_ldm
    import train_vae
    from adm_amd.ddm import datasets, depth_data
    assert depth_data.DEPTH_CLASSES == (FULL, SHORT)
    monkeypatch.setattr(depth_data.DepthBatchStream, "__init__", lambda self, *a, **k: None)
    for cfg in ({"class_name": FULL}, {"class_name": SHORT}, {"class_name": "synthetic", "synthetic_of": FULL}):
        assert datasets.dataset_of(cfg) == FULL
        assert type(train_cond_ldm.batch_stream(cfg, 2, (32, 32), "cpu", 0)) is depth_data.DepthBatchStream
        first = train_vae.first_stage_stream(cfg, 2, (32, 32), "cpu", 0)
        assert type(first) is depth_data.DepthMapStream and first.channels == 1 and "channels" not in first.__dict__
        assert sample_cond_ldm.sampling_dataset(cfg) == FULL
        with pytest.raises(NotImplementedError, match="the pixel-space conditional sampler reads ddm.data.DUTSDataset"):
            sample_cond_dpm.check_dataset(cfg)
    sm = datasets.DATASETS[FULL].sampling
    assert sm.form == "slide" and sm.depth and sm.gray and not sm.psnr and sm.synthetic and "split: test" in sm.split_test
    assert sm.item(None, 0, {"ori_size": [(426, 560)], "img_name": ["rgb_00045.jpg"]}) == ((426, 560), "rgb_00045.png")
    # the fields appended to Sampling have defaults: no other row changed
    assert [k for k, d in datasets.DATASETS.items() if d.sampling and d.sampling.depth] == [FULL]
    assert datasets.SR_SAMPLING.depth is False
    # the resize variant stays refused everywhere
    for name in ("ddm.data.NYUDv2DepthDataset2", "NYUDv2DepthDataset2"):
        assert datasets.dataset_of({"class_name": name}) is None
    # a sampler without split: test is refused with the entry's message
    with pytest.raises(ValueError, match="needs data.split: test"):
        sample_cond_ldm.DatasetCondStream(datasets.DATASETS[FULL], {"class_name": FULL, "split": "train"}, 1, (32, 32), "cpu", 0)
    # sliding windows of the recipe: 2 x 3 windows of 320x320 at stride 160 over a 426x560 frame
    wins = sample_cond_ldm.slide_windows(426, 560, (320, 320), (160, 160))
    assert wins == [(0, 320, 0, 320), (0, 320, 160, 480), (0, 320, 240, 560), (106, 426, 0, 320), (106, 426, 160, 480), (106, 426, 240, 560)]


def test_header_and_ctypes_table_agree_for_the_new_entry_points():
    from adm_amd import hip
    header = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    for name in ("adm_depth_batch", "adm_depth_metrics", "adm_depth_metrics_blocks"):
        m = re.search(r"^(?:int|long)\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.M | re.S)
        assert m, name
        assert len(hip._SIGS[name]) == m.group(1).count(",") + 1, name
    assert "adm_depth_metrics_blocks" in hip.NO_STREAM and "adm_depth_batch" not in hip.NO_STREAM
    lib = hip.lib()
    assert lib.adm_depth_metrics_blocks(1) == 1 and lib.adm_depth_metrics_blocks(4096) == 1 and lib.adm_depth_metrics_blocks(4097) == 2
    assert lib.adm_depth_metrics_blocks(426 * 560) == 59 and lib.adm_depth_metrics_blocks(10 ** 7) == 64
    assert lib.adm_depth_metrics_blocks(0) == -22
    src = open(os.path.join(ROOT, "adm_amd", "csrc", "Makefile")).read()
    assert " depth_data.hip" in src and "FLAGS_depth_data" not in src


def test_16_bit_png_round_trip(tmp_path):
    from PIL import Image
    from adm_amd.ddm.depth_data import read_depth_png, write_depth_png
    units = np.asarray([[0, 1, 9999], [10000, 65535, 256]], dtype=np.uint16)
    path = tmp_path / "d.png"
    write_depth_png(path, units)
    im = Image.open(path)
    assert im.mode == "I;16" and im.size == (3, 2)
    back = read_depth_png(path)
    assert back.dtype == np.uint16 and np.array_equal(back, units)
    with pytest.raises(ValueError, match="expected uint16"):
        write_depth_png(path, units.astype(np.int32))
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(tmp_path / "rgb.png")
    with pytest.raises(ValueError, match="one-channel integer depth image"):
        read_depth_png(tmp_path / "rgb.png")


def test_metric_definitions_on_a_hand_computed_case():
    """2x2 of fractions that float32 holds exactly; metres g = (2.5, 5, 0 -> invalid, 5), p = (3.125, 2.5, 7, 5): by hand
    abs_rel = (0.25 + 0.5 + 0) / 3, sq_rel = (0.15625 + 1.25 + 0) / 3, rmse = sqrt((0.390625 + 6.25) / 3), ratios (1.25, 2, -, 1) ->
    d1 = 1/3 (1.25 is not < 1.25), d2 = 2/3, d3 = 2/3 (2 is not < 1.953125)."""
    from adm_amd.metrics import depth as M
    gt = np.asarray([[[[0.25, 0.5], [0.0, 0.5]]]], dtype=np.float32)
    pred = np.asarray([[[[0.3125, 0.25], [0.7, 0.5]]]], dtype=np.float32)
    s = R.sums(pred, gt)
    assert s.shape == (1, 10) and s[0, 0] == 3
    g, p = np.asarray([2.5, 5.0, 5.0]), np.asarray([3.125, 2.5, 5.0])
    e = np.log(p) - np.log(g)
    want = {"abs_rel": (0.25 + 0.5) / 3, "sq_rel": (0.15625 + 1.25) / 3, "rmse": np.sqrt(6.640625 / 3), "rmse_log": np.sqrt((e ** 2).mean()),
            "silog": 100 * np.sqrt((e ** 2).mean() - e.mean() ** 2), "log10": np.abs(np.log10(p / g)).mean(), "d1": 1 / 3, "d2": 2 / 3,
            "d3": 2 / 3}
    for res in (R.metrics(s), M.metrics_from_sums(s)):
        assert res["images"] == 1 and res["skipped"] == 0
        for k, v in want.items():
            assert res[k] == pytest.approx(v, rel=1e-12), k
    assert tuple(M.KEYS) == tuple(R.KEYS) == tuple(want)
    # the prediction is clamped to the range, and an image without a valid pixel is skipped, not averaged in
    gt2 = np.concatenate([gt, np.zeros_like(gt), np.full_like(gt, 1.0)])
    pred2 = np.concatenate([np.asarray([[[[0.3125, 0.25], [0.7, 2.0]]]], dtype=np.float32), pred, pred])
    s2 = R.sums(pred2, gt2)
    assert s2[1, 0] == 0 and s2[2, 0] == 0          # zeros, and gt exactly at max_depth
    assert s2[0, 3] == 0.390625 + 6.25 + 25          # 20 m clamped to 10 m against 5 m
    for res in (R.metrics(s2), M.metrics_from_sums(s2)):
        assert res["images"] == 1 and res["skipped"] == 2 and np.isfinite(res["rmse"])
    none = M.metrics_from_sums(s2[1:])
    assert none["images"] == 0 and none["skipped"] == 2 and np.isnan(none["abs_rel"])
    # R.metrics and metrics_from_sums agree on a larger draw
    rng = np.random.default_rng(0)
    g3 = rng.uniform(0.05, 0.95, (3, 1, 9, 11)).astype(np.float32)
    p3 = (g3 * np.exp(rng.normal(0, 0.25, g3.shape))).astype(np.float32)
    a, b = R.metrics(R.sums(p3, g3)), M.metrics_from_sums(R.sums(p3, g3))
    assert all(a[k] == pytest.approx(b[k], rel=1e-12) for k in a)


def test_full_frames_would_not_survive_the_first_stage():
    """The reference's ``split: full`` skips the crop, so its autoencoder would see 426x560 frames: two stride-2 convolutions with
    (0, 1, 0, 1) padding take 426 rows to 213 and 106, and two nearest x2 upsamplings give 424 back -- the reconstruction loss would
    compare 424 rows with 426.  (Why every split but 'test' is cropped here.)"""
    import torch.nn.functional as F
    x = torch.zeros(1, 1, 426, 560)
    w = torch.zeros(1, 1, 3, 3)
    h1 = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
    h2 = F.conv2d(F.pad(h1, (0, 1, 0, 1)), w, stride=2)
    up = F.interpolate(F.interpolate(h2, scale_factor=2.0, mode="nearest"), scale_factor=2.0, mode="nearest")
    assert tuple(h1.shape[2:]) == (213, 280) and tuple(h2.shape[2:]) == (106, 140) and tuple(up.shape[2:]) == (424, 560)


def test_shipped_yamls_hold_the_reference_values():
    import yaml
    load = lambda n: yaml.load(open(os.path.join(ROOT, "configs", "depth_estimation", n)), Loader=yaml.SafeLoader)
    ae, train, sample = load("nyud_ae_kl_320x320.yaml"), load("nyud_cond_ddm_const_ldm.yaml"), load("nyud_cond_ddm_const_ldm_sample.yaml")
    for cfg in (ae, train, sample):
        assert cfg["data"]["class_name"] == "synthetic" and cfg["data"]["synthetic_of"] == FULL and not cfg["data"]["data_root"]
        assert cfg["data"]["image_size"] == [320, 320] and cfg["data"]["batch_size"] == 8
    dd = ae["model"]["ddconfig"]
    assert dd["in_channels"] == dd["out_ch"] == ae["model"]["lossconfig"]["disc_in_channels"] == 1 and dd["resolution"] == [320, 320]
    assert ae["data"]["split"] == "full" and ae["trainer"]["lr"] == 5e-6 and ae["trainer"]["train_num_steps"] == 100000
    for cfg in (train, sample):
        m, u = cfg["model"], cfg["model"]["unet"]
        assert m["class_name"] == "ddm.ddm_const.LatentDiffusion" and m["use_l1"] is True and m["scale_factor"] == 0.3
        assert "use_disloss" not in m and "loss_main" not in m
        assert m["first_stage"]["ddconfig"] == dd
        assert u["class_name"] == "unet.cond_unet.Unet" and u["dim"] == 128 and u["dim_mults"] == [1, 2, 4, 4]
        assert u["cond_encoder"] == "swin_b" and u["train_cond_encoder"] is True
    assert train["data"]["split"] == "train" and train["trainer"]["gradient_accumulate_every"] == 2
    assert train["trainer"]["train_num_steps"] == 300000 and train["trainer"]["ema_update_every"] == 8
    s = sample["sampler"]
    assert sample["data"]["split"] == "test" and s["crop_size"] == [320, 320] and s["stride"] == [160, 160]
    assert s["flip_test"] is True and s["out_channels"] == 1 and s["cond_encoder"] == "swin_b" and not s.get("depth_png8")
