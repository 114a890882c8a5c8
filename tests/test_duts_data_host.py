"""CPU: the host half of the saliency pairs (adm_amd/ddm/pair_data.py) -- the NumPy restatement against PIL's own bytes
(tests/golden/g23_duts_data.npz, tools/make_golden_duts.py), the table pool, DUTS file discovery, the LDS budget, the dispatch of
train_cond_ldm.batch_stream, the committed YAMLs and save_grid's one-channel path.  PIL's resize is integer arithmetic, so every
comparison of bytes is for ZERO differences."""
import os

import numpy as np
import pytest
import torch
import yaml

import duts_data_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g23_duts_data.npz")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def test_restatement_reproduces_every_golden_output(g):
    assert tuple(g["target"]) == R.TARGET and g["sizes"].tolist() == [[list(p), list(m)] for p, m in R.CASES]
    assert g["draws"].tolist() == [list(d) for d in R.DRAWS]
    n = 0
    for i in range(len(R.CASES)):
        photo, gmap = R.case_sources(i)
        assert [int(photo.astype(np.int64).sum()), int(gmap.astype(np.int64).sum())] == g[f"c{i}.checksum"].tolist(), i
        rgb, gray = R.duts_pair(photo, gmap, R.TARGET)
        assert np.array_equal(rgb, g[f"c{i}.rgb"]) and np.array_equal(gray, g[f"c{i}.gray"]), i
        if f"c{i}.rgb_flipped" in g.files:
            rgb, gray = R.duts_pair(photo, gmap, R.TARGET, flip=True)
            assert np.array_equal(rgb, g[f"c{i}.rgb_flipped"]) and np.array_equal(gray, g[f"c{i}.gray_flipped"]), i
            n += 1
    assert n == len({i for i, f in R.DRAWS if f}) == 2
    rgb, gray = R.duts_pair(g["edge.photo"], g["edge.map"], (16, 24))
    assert np.array_equal(rgb, g["edge.rgb"]) and np.array_equal(gray, g["edge.gray"])
    # ... and there PIL's uint8 intermediate shows: one rounding at the end gives other bytes
    once = R.resize_rounded_once(g["edge.photo"], (16, 24))
    assert int((once != g["edge.rgb"]).sum()) == int(g["edge.differing"][0]) > 0


def test_identity_table_copies_and_upscaling_has_three_taps():
    from adm_amd.ddm.sr_data import resample_table
    bounds, coeffs = resample_table(40, 40, "bilinear")
    assert coeffs.shape == (40, 3) and all(int(coeffs[i, :bounds[i, 1]].sum()) == 1 << 22 for i in range(40))
    x = R.hash_bytes((40, 56, 3), "duts.identity")
    assert np.array_equal(R.resize_rgb(x, (40, 56)), x)          # the identity through both passes, no shortcut needed
    assert resample_table(37, 40, "bilinear")[1].shape[1] == 3 and resample_table(100, 40, "bilinear")[1].shape[1] == 7


def test_table_pool_shares_tables_and_round_trips():
    from adm_amd.ddm.pair_data import build_table_pool, read_table, taps
    from adm_amd.ddm.sr_data import resample_table
    H, W = 40, 56
    rgb_hw = np.array([[37, 53], [97, 53], [100, 140]])          # images 0 and 1 share their width; image 2 is 2.5x in both axes
    gray_hw = np.array([[37, 53], [89, 140], [100, 140]])        # image 1's map has another size than its photo
    p = build_table_pool(rgb_hw, gray_hw, (H, W))
    t = p["img_tab"]
    assert t.shape == (3, 4) and t.dtype == np.int32 and p["tab"].dtype == np.int32 and p["dir"].dtype == np.int32
    assert t[0, 0] == t[1, 0] and t[0, 1] != t[1, 1]             # one width table for two images of one width
    assert t[0, 0] == t[0, 2] and t[0, 1] == t[0, 3]             # a map of its photo's size shares both tables
    assert t[1, 2] == t[2, 0] == t[2, 2] and t[1, 3] != t[1, 1]
    # (53 -> 56), (37 -> 40), (97 -> 40), (140 -> 56), (89 -> 40), (100 -> 40)
    assert p["keys"] == [(53, 56), (37, 40), (97, 40), (140, 56), (89, 40), (100, 40)] and p["dir"].shape == (6, 2)
    total = 0
    for tid, (n_in, n_out) in enumerate(p["keys"]):
        bounds, coeffs = resample_table(n_in, n_out, "bilinear")
        got_b, got_c = read_table(p, tid, n_out)
        assert np.array_equal(got_b, bounds) and np.array_equal(got_c, coeffs), (n_in, n_out)
        assert p["dir"][tid].tolist() == [total, coeffs.shape[1]] and taps(n_in, n_out) == coeffs.shape[1]
        total += bounds.size + coeffs.size
    assert total == p["tab"].size
    k = {key: int(p["dir"][i, 1]) for i, key in enumerate(p["keys"])}
    assert k[(37, 40)] == 3 and k[(53, 56)] == 3 and k[(100, 40)] == 7 and k[(140, 56)] == 7          # up-scaling: 3 taps; 2.5x: 7


def test_pack_bytes_layout():
    from adm_amd.ddm.pair_data import pack_bytes
    maps = [np.full((3, 5), 7, np.uint8), np.full((2, 3), 9, np.uint8)]
    flat, off, hw = pack_bytes(maps, 1, "map")
    assert flat.size == 24 and off.tolist() == [0, 15] and hw.tolist() == [[3, 5], [2, 3]] and off.dtype == np.int64
    assert flat[:15].tolist() == [7] * 15 and flat[15:21].tolist() == [9] * 6 and not flat[21:].any()          # dword padding
    with pytest.raises(ValueError, match="map 1"):
        pack_bytes([maps[0], np.zeros((2, 3, 3), np.uint8)], 1, "map")
    with pytest.raises(ValueError, match="photo 0"):
        pack_bytes([maps[0]], 3, "photo")


def duts_tree(root, split_dir, sizes, tag):
    """A folder laid out as DUTS: <root>/<split_dir>/<split_dir>-Image/*.jpg and .../<split_dir>-Mask/*.png."""
    from PIL import Image
    img_dir, mask_dir = root / split_dir / f"{split_dir}-Image", root / split_dir / f"{split_dir}-Mask"
    img_dir.mkdir(parents=True), mask_dir.mkdir(parents=True)
    names = []
    for i, ((ph, pw), (mh, mw)) in enumerate(sizes):
        name = f"{tag}_{len(sizes) - i:04d}"          # written in reverse order: discovery must sort
        Image.fromarray(R.hash_bytes((ph, pw, 3), f"{tag}.p{i}")).save(img_dir / f"{name}.jpg", quality=95)
        Image.fromarray(R.hash_bytes((mh, mw), f"{tag}.m{i}")).save(mask_dir / f"{name}.png")
        names.append(f"{name}.jpg")
    return sorted(names)


def test_file_discovery_and_missing_map(tmp_path):
    from PIL import Image
    from adm_amd.ddm.pair_data import find_duts_pairs, load_duts
    tr = duts_tree(tmp_path, "DUTS-TR", [((30, 44), (30, 44)), ((50, 36), (48, 40)), ((33, 33), (33, 33))], "tr")
    te = duts_tree(tmp_path, "DUTS-TE", [((40, 40), (40, 40))], "te")
    pairs = find_duts_pairs(str(tmp_path), "train")
    assert [p.name for p, _ in pairs] == tr
    for p, m in pairs:
        assert p.parent.name == "DUTS-TR-Image" and m.parent.name == "DUTS-TR-Mask" and m.name == p.name.replace(".jpg", ".png")
    assert [p.name for p, _ in find_duts_pairs(str(tmp_path), "test")] == te
    photos, maps, names = load_duts(str(tmp_path), "train")
    assert names == tr and [a.shape for a in photos] == [(33, 33, 3), (50, 36, 3), (30, 44, 3)]
    assert [a.shape for a in maps] == [(33, 33), (48, 40), (30, 44)] and all(a.dtype == np.uint8 for a in photos + maps)
    assert np.array_equal(maps[2], np.asarray(Image.open(tmp_path / "DUTS-TR" / "DUTS-TR-Mask" / "tr_0003.png").convert("L")))
    (tmp_path / "DUTS-TR" / "DUTS-TR-Mask" / "tr_0002.png").unlink()
    with pytest.raises(FileNotFoundError, match="tr_0002.png"):
        find_duts_pairs(str(tmp_path), "train")
    with pytest.raises(FileNotFoundError, match="no jpg"):
        find_duts_pairs(str(tmp_path / "DUTS-TE" / "DUTS-TE-Mask"), "other")


def test_an_image_beyond_the_supported_ratio_is_refused_by_name():
    from adm_amd.ddm.pair_data import LDS_BUDGET, PairPool, lds_need
    out = (40, 56)
    assert lds_need(out, 160, 224) <= 20 * 1024                  # ratio 4: about 19 KB
    assert lds_need(out, 7 * 40, 7 * 56) <= LDS_BUDGET < lds_need(out, 8 * 40, 8 * 56)          # the limit is near 7
    ok = np.zeros((160, 224, 3), np.uint8)
    pool = PairPool.from_arrays([ok], [ok[:, :, 0]], out, CPU, ["fits.jpg"])
    assert (pool.max_h, pool.max_w, pool.kv, pool.kh) == (160, 224, 9, 9) and pool.n == 1
    big = np.zeros((9 * 40, 9 * 56, 3), np.uint8)
    with pytest.raises(ValueError, match=r"pair 1 \(huge\.jpg\): its photo is 360x504"):
        PairPool.from_arrays([ok, big], [ok[:, :, 0], ok[:, :, 0]], out, CPU, ["fits.jpg", "huge.jpg"])
    with pytest.raises(ValueError, match=r"pair 0: its map is 360x504"):
        PairPool.from_arrays([ok], [big[:, :, 0]], out, CPU)
    # a tall and a wide image that fit one by one but not in one capacity
    tall, wide = np.zeros((7 * 40, 56, 3), np.uint8), np.zeros((40, 13 * 56, 3), np.uint8)
    assert lds_need(out, 280, 56) <= LDS_BUDGET and lds_need(out, 40, 728) <= LDS_BUDGET < lds_need(out, 280, 728)
    with pytest.raises(ValueError, match=r"pair 0 \(tall\) \(280 rows\) and pair 1 \(wide\) \(728 columns\) together"):
        PairPool.from_arrays([tall, wide], [tall[:, :, 0], wide[:, :, 0]], out, CPU, ["tall", "wide"])


def test_lds_sizing_is_what_it_was_before_the_resampler_was_shared():
    """adm_pair_resize_lds(H, W, max_h, max_w, kh, kv) as the library returned it when pair_data.hip still sized its LDS itself:
    the shapes of the test above, and the 384x384 recipe from 420x420 and 400x300 sources."""
    from adm_amd import hip
    from adm_amd.ddm.pair_data import lds_need, taps
    was = {(40, 56, 160, 224, 9, 9): 19632, (40, 56, 280, 392, 15, 15): 52256, (40, 56, 320, 448, 17, 17): 66760,
           (40, 56, 280, 56, 3, 15): 14220, (40, 56, 40, 728, 27, 3): 15600, (40, 56, 280, 728, 27, 15): 89808,
           (40, 56, 360, 504, 19, 19): 82412, (24, 40, 216, 360, 19, 19): 82412, (384, 384, 420, 420, 5, 5): 3400,
           (384, 384, 400, 300, 3, 5): 2712}
    for (H, W, max_h, max_w, kh, kv), want in was.items():
        assert (taps(max_w, W), taps(max_h, H)) == (kh, kv)
        assert hip.lib().adm_pair_resize_lds(H, W, max_h, max_w, kh, kv) == want == lds_need((H, W), max_h, max_w), (H, W, max_h, max_w)
    assert hip.lib().adm_pair_resize_lds(40, 56, 160, 224, 0, 9) == -22


def test_batch_stream_dispatch(tmp_path):
    from adm_amd.ddm.pair_data import DUTSBatchStream
    from adm_amd.ddm.sr_data import SRBatchStream
    from train_cond_ldm import batch_stream
    duts_tree(tmp_path, "DUTS-TR", [((30, 44), (30, 44)), ((50, 36), (48, 40))], "tr")
    for cfg in ({"class_name": "ddm.data.DUTSDataset", "data_root": str(tmp_path)},
                {"class_name": "DUTSDataset", "data_root": str(tmp_path)},
                {"class_name": "synthetic", "synthetic_of": "ddm.data.DUTSDataset"}):
        s = batch_stream(cfg, 2, (32, 48), CPU, 1)
        assert type(s) is DUTSBatchStream and s.pool.out_hw == (32, 48), cfg
    assert s.pool.n == DUTSBatchStream.SYNTHETIC_PAIRS
    hw = s.pool.hw_host[0]
    assert (hw[:, 0] < 32).any() and (hw[:, 0] > 32).any() and (hw[:, 1] < 48).any() and (hw[:, 1] > 48).any()
    assert type(batch_stream({"class_name": "synthetic"}, 2, (32, 32), CPU, 1)) is SRBatchStream          # the other routes are unchanged
    with pytest.raises(ValueError, match="data_root"):
        batch_stream({"class_name": "ddm.data.DUTSDataset"}, 2, (32, 48), CPU, 1)
    with pytest.raises(NotImplementedError):
        DUTSBatchStream({"class_name": "ddm.data.SketchDataset"}, 2, (32, 48), CPU, 1)
    with pytest.raises(NotImplementedError, match="split"):
        DUTSBatchStream({"class_name": "synthetic", "synthetic_of": "DUTSDataset", "split": "val"}, 2, (32, 48), CPU, 1)


def test_committed_yamls_carry_the_recipe():
    for name, sample in (("duts_cond_ddm_const_ldm.yaml", False), ("duts_cond_ddm_const_ldm_sample.yaml", True)):
        cfg = yaml.load(open(os.path.join(ROOT, "configs", "saliency", name)), Loader=yaml.SafeLoader)
        m, u, fs, d, t = cfg["model"], cfg["model"]["unet"], cfg["model"]["first_stage"], cfg["data"], cfg["trainer"]
        assert m["class_name"] == "ddm.ddm_const.LatentDiffusion" and m["image_size"] == [384, 384] and m["sampling_timesteps"] == 10
        assert m["use_l1"] is True and m["weighting_loss"] is True and m["scale_factor"] == 0.25 and m["scale_by_std"] is True
        assert m["default_scale"] is True and m["eps"] == 1e-4 and m["sigma_min"] == 0.01 and m["start_dist"] == "normal"
        dd = fs["ddconfig"]
        assert fs["class_name"] == "ddm.encoder_decoder.AutoencoderKL" and fs["embed_dim"] == 3 and not fs["ckpt_path"]
        assert (dd["in_channels"], dd["out_ch"], dd["ch"], dd["ch_mult"], dd["z_channels"]) == (1, 1, 128, [1, 2, 4], 3)
        assert dd["resolution"] == [384, 384] and dd["num_res_blocks"] == 2 and fs["lossconfig"]["disc_in_channels"] == 1
        assert u["class_name"] == "unet.cond_unet.Unet" and u["dim"] == 128 and u["dim_mults"] == [1, 2, 4, 4] and u["channels"] == 3
        assert u["cond_feature_size"] == [96, 96] and u["window_sizes1"] == u["window_sizes2"] == [[8, 8], [4, 4], [2, 2], [1, 1]]
        assert u["fix_bb"] is False and u["cond_encoder"] == "swin_b" and u["train_cond_encoder"] is True
        assert "cond_encoder_weights" in u and not u["cond_encoder_weights"]
        assert d["image_size"] == [384, 384] and not d["data_root"]
        assert (t["gradient_accumulate_every"], t["lr"], t["min_lr"], t["train_num_steps"]) == (2, 5e-5, 5e-6, 300000)
        assert t["ema_update_after_step"] == 20000 and t["ema_update_every"] == 8 and t["test_before"] is True
        assert not os.path.isabs(t["results_folder"])
        if sample:
            s = cfg["sampler"]
            assert d["class_name"] == "ddm.data.DUTSDataset" and d["split"] == "test" and d["augment_horizontal_flip"] is False
            assert s["out_channels"] == 1 and s["crop_size"] == s["stride"] == [384, 384] and s["sample_num"] == 100
            assert s["use_ema"] is True and s["cond_encoder"] == "swin_b"
            assert not os.path.isabs(s["ckpt_path"]) and not os.path.isabs(s["save_folder"])
        else:
            assert d["class_name"] == "synthetic" and d["synthetic_of"] == "ddm.data.DUTSDataset" and d["split"] == "train"
            assert d["batch_size"] == 8 and d["augment_horizontal_flip"] is True


def test_save_grid_one_channel_is_mode_l_and_three_channels_are_unchanged(tmp_path):
    from PIL import Image
    from train_uncond_dpm import save_grid
    g1 = torch.from_numpy(R.hash_bytes((3, 1, 6, 5), "grid.l").astype(np.float32)) / 255
    save_grid(g1, str(tmp_path / "l.png"), 2)
    im = Image.open(tmp_path / "l.png")
    assert im.mode == "L" and im.size == (10, 12)          # 3 images in 2 columns: 2 rows of 6, 2 columns of 5
    a = np.asarray(im)
    u = (g1.clamp(0, 1) * 255).round().to(torch.uint8).numpy()
    assert np.array_equal(a[:6, :5], u[0, 0]) and np.array_equal(a[:6, 5:], u[1, 0]) and np.array_equal(a[6:, :5], u[2, 0])
    assert not a[6:, 5:].any()
    # three channels: the bytes of the formula save_grid had before the one-channel path existed
    g3 = torch.from_numpy(R.hash_bytes((3, 3, 6, 5), "grid.rgb").astype(np.float32)) / 255 * 1.2 - 0.1          # clamps on both sides
    save_grid(g3, str(tmp_path / "rgb.png"), 2)
    img = (g3.clamp(0, 1) * 255).round().to(torch.uint8).cpu()
    canvas = torch.zeros(3, 2 * 6, 2 * 5, dtype=torch.uint8)
    for i in range(3):
        r, c = divmod(i, 2)
        canvas[:, r * 6:(r + 1) * 6, c * 5:(c + 1) * 5] = img[i]
    Image.fromarray(canvas.permute(1, 2, 0).numpy()).save(tmp_path / "old.png")
    assert open(tmp_path / "rgb.png", "rb").read() == open(tmp_path / "old.png", "rb").read()
    assert Image.open(tmp_path / "rgb.png").mode == "RGB"
