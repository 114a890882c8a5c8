"""CPU-only checks of the first-stage data path and of the one-channel autoencoder cases: the table pool of a one-plane pool, the
LDS budget refusal, file discovery of the three sources, train_vae.first_stage_stream's dispatch and refusals, the channel checks,
the argument checks of adm_image_resize_batch (which precede its launch: every call here is refused, none reaches a device), and
the plain-PyTorch restatement (tests/ae_train_c1_ref.py) against the reference's fp64 results for AutoencoderKL(in_channels=1,
out_ch=1) (tests/golden/g27_ae_train_c1.npz), with fp32 torch's own deviation on the same inputs.  No GPU call is made here: the
streams are built on the CPU device, where only their launch would fail."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import ae_train_c1_ref as R1
import lpips_ref
from sr_data_ref import hash_bytes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------ tables and budget
def test_table_pool_of_repeated_sizes():
    """Equal (in, out) pairs share one table whichever image or axis they come from; img_tab names (width table, height table)."""
    from adm_amd.ddm.image_data import build_plane_tables
    from adm_amd.ddm.pair_data import read_table
    from adm_amd.ddm.sr_data import resample_table
    hw = [(30, 44), (44, 30), (30, 44), (32, 32), (50, 32)]
    pool = build_plane_tables(hw, (32, 32))
    # first use, in (width, height) order per image: 44->32, 30->32, [30->32, 44->32 again], [again], 32->32, [32->32], 50->32
    assert pool["keys"] == [(44, 32), (30, 32), (32, 32), (50, 32)]
    assert pool["img_tab"].dtype == np.int32 and pool["img_tab"].tolist() == [[0, 1], [1, 0], [0, 1], [2, 2], [2, 3]]
    assert pool["dir"].shape == (4, 2) and pool["tab"].dtype == np.int32
    total = 0
    for t, (i, o) in enumerate(pool["keys"]):
        bounds, coeffs = resample_table(i, o, "bilinear")
        assert pool["dir"][t].tolist() == [total, coeffs.shape[1]]
        b, c = read_table(pool, t, o)
        assert np.array_equal(b, bounds) and np.array_equal(c, coeffs)
        total += bounds.size + coeffs.size
    assert pool["tab"].size == total
    # a non-square target keeps the axes apart: 40 -> 24 (width) and 40 -> 40 (height) are two tables
    p2 = build_plane_tables([(40, 40)], (40, 24))
    assert p2["keys"] == [(40, 24), (40, 40)] and p2["img_tab"].tolist() == [[0, 1]]


def test_plane_pool_on_the_host_and_budget_refusal():
    from adm_amd.ddm import image_data as I
    from adm_amd.ddm.pair_data import LDS_BUDGET, lds_need, taps
    imgs = [hash_bytes((29, 37), "host.a"), hash_bytes((30, 38), "host.b"), hash_bytes((9, 11), "host.c")]
    pool = I.PlanePool.from_arrays(imgs, (32, 32), CPU, names=["a.png", "b.png", "c.png"])
    assert pool.channels == 1 and pool.n == 3 and pool.flat.numel() % 4 == 0 and pool.flat.numel() >= 29 * 37 + 30 * 38 + 99
    assert pool.off.tolist() == [0, 29 * 37, 29 * 37 + 30 * 38] and pool.hw.tolist() == [[29, 37], [30, 38], [9, 11]]
    assert (pool.max_h, pool.max_w) == (30, 38) and (pool.kh, pool.kv) == (taps(38, 32), taps(30, 32))
    assert pool.nbytes == pool.flat.numel() + 4 * pool.tab.numel()
    rgb = I.PlanePool.from_arrays([hash_bytes((20, 24, 3), "host.rgb")], (32, 32), CPU)
    assert rgb.channels == 3 and rgb.flat.numel() == 20 * 24 * 3
    # mixed planes, an empty pool, a channel count that is neither
    with pytest.raises(ValueError, match="image 1"):
        I.PlanePool.from_arrays([imgs[0], hash_bytes((8, 8, 3), "host.mixed")], (32, 32), CPU)
    with pytest.raises(ValueError, match="empty"):
        I.PlanePool.from_arrays([], (32, 32), CPU)
    with pytest.raises(ValueError, match="1 or 3"):
        I.PlanePool(pool.flat, [0], [(4, 4)], 2, (32, 32), CPU)
    # a source above about 7x the target per axis is refused by name, before anything is copied
    assert lds_need((32, 32), 7 * 32, 7 * 32) <= LDS_BUDGET < lds_need((32, 32), 9 * 32, 9 * 32)
    big = np.zeros((9 * 32, 9 * 32), dtype=np.uint8)
    with pytest.raises(ValueError, match=r"image 1 \(huge\.png\): it is 288x288, 9\.00 x 9\.00 times the 32x32 target.*budget is 65536"):
        I.PlanePool.from_arrays([imgs[0], big], (32, 32), CPU, names=["a.png", "huge.png"])
    with pytest.raises(ValueError, match="image 0: it is 288x288"):
        I.PlanePool.from_uniform_draws([(288, 288)], 1, (32, 32), CPU, torch.Generator().manual_seed(0))
    # tall and wide sources that fit one by one but not together: both are named
    tall, wide = (13 * 32, 32), (32, 13 * 32)
    assert lds_need((32, 32), *tall) <= LDS_BUDGET and lds_need((32, 32), *wide) <= LDS_BUDGET < lds_need((32, 32), tall[0], wide[1])
    with pytest.raises(ValueError, match=r"image 0 \(416 rows\) and image 1 \(416 columns\) together"):
        I.check_plane_budget([tall, wide], (32, 32))


# ------------------------------------------------------------------------------------------------ discovery
def _png(path, shape, tag):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(hash_bytes(shape, tag)).save(path)


def test_file_discovery_of_the_three_sources(tmp_path):
    from PIL import Image
    from adm_amd.ddm import image_data as I
    # ImageDataset: *.jpg then *.png of the folder itself, each sorted; nothing below it
    folder = tmp_path / "folder"
    for name in ("b.png", "a.png", "sub/c.png"):
        _png(folder / name, (12, 10, 3), name)
    Image.fromarray(hash_bytes((12, 10, 3), "z.jpg")).save(folder / "z.jpg", quality=90)
    (folder / "notes.txt").write_text("x")
    assert [p.name for p in I.find_images(str(folder))] == ["z.jpg", "a.png", "b.png"]
    with pytest.raises(FileNotFoundError, match="no jpg/png image in"):
        I.find_images(str(tmp_path / "folder" / "sub" / "none"))
    s = I.ImageFolderStream({"class_name": "ddm.data.ImageDataset", "img_folder": str(folder)}, 2, (16, 16), CPU, 0)
    assert s.channels == 3 and s.pool.n == 3 and s.pool.names == ["z.jpg", "a.png", "b.png"] and s.flip is False
    assert I.ImageFolderStream({"class_name": "ImageDataset", "img_folder": str(folder), "augment_horizontal_flip": True}, 2, (16, 16),
                               CPU, 0).flip is True
    # DUTSDataset: the maps, located through their photos; the photos are stubs no decoder could read
    duts = tmp_path / "duts"
    for i, hw in enumerate([(20, 30), (31, 17)]):
        (duts / "DUTS-TR" / "DUTS-TR-Image").mkdir(parents=True, exist_ok=True)
        (duts / "DUTS-TR" / "DUTS-TR-Image" / f"im{i}.jpg").write_bytes(b"not an image")
        _png(duts / "DUTS-TR" / "DUTS-TR-Mask" / f"im{i}.png", hw, f"duts.map{i}")
    s = I.DUTSMapStream({"class_name": "ddm.data.DUTSDataset", "data_root": str(duts), "augment_horizontal_flip": True}, 2, (16, 16), CPU, 0)
    assert s.channels == 1 and s.pool.channels == 1 and s.pool.names == ["im0.png", "im1.png"] and s.flip is True
    assert s.pool.hw_host.tolist() == [[20, 30], [31, 17]]
    back = np.asarray(Image.open(duts / "DUTS-TR" / "DUTS-TR-Mask" / "im1.png").convert("L"))
    o = int(s.pool.off[1])
    assert np.array_equal(s.pool.flat[o:o + 31 * 17].numpy().reshape(31, 17), back)
    (duts / "DUTS-TR" / "DUTS-TR-Mask" / "im1.png").write_bytes(b"broken")
    with pytest.raises(OSError, match="im1.png cannot be read as an image"):
        I.DUTSMapStream({"class_name": "ddm.data.DUTSDataset", "data_root": str(duts)}, 2, (16, 16), CPU, 0)
    # SketchDataset: the photos below GT/train, located with their sketches, which are stubs
    sk = tmp_path / "sketch"
    for i in range(2):
        _png(sk / "GT" / "train" / "cat" / f"p{i}.png", (14, 18, 3), f"sk.photo{i}")
        (sk / "Sketch" / "train" / "cat").mkdir(parents=True, exist_ok=True)
        (sk / "Sketch" / "train" / "cat" / f"p{i}.png").write_bytes(b"not an image")
    s = I.SketchPhotoStream({"class_name": "ddm.data.SketchDataset", "data_root": str(sk)}, 2, (16, 16), CPU, 0)
    assert s.channels == 3 and s.pool.n == 2 and s.pool.names == ["p0.png", "p1.png"] and s.flip is False
    # a class without its root key raises and names the key
    for cls, name, key in ((I.ImageFolderStream, "ddm.data.ImageDataset", "img_folder"), (I.DUTSMapStream, "ddm.data.DUTSDataset", "data_root"),
                           (I.SketchPhotoStream, "ddm.data.SketchDataset", "data_root")):
        with pytest.raises(ValueError, match=f"{name} needs data.{key}"):
            cls({"class_name": name}, 2, (16, 16), CPU, 0)
        with pytest.raises(NotImplementedError, match=f"only {name}"):
            cls({"class_name": "ddm.data.CelebAHQ"}, 2, (16, 16), CPU, 0)


# ------------------------------------------------------------------------------------------------ drivers
def test_first_stage_stream_dispatch_and_refusals(tmp_path, capsys):
    import train_uncond_dpm as U
    import train_vae as T
    from adm_amd.ddm import image_data as I
    from adm_amd.ddm.sr_data import SRBatchStream
    for of, cls, ch in (("ddm.data.ImageDataset", I.ImageFolderStream, 3), ("ddm.data.DUTSDataset", I.DUTSMapStream, 1),
                        ("ddm.data.SketchDataset", I.SketchPhotoStream, 3)):
        s = T.first_stage_stream({"class_name": "synthetic", "synthetic_of": of, "synthetic_sizes": [[20, 30], [40, 28], [20, 30]]}, 2,
                                 (32, 32), CPU, 5)
        assert type(s) is cls and s.channels == ch and s.pool.n == 3 and s.pool.channels == ch
        assert s.pool.hw_host.tolist() == [[20, 30], [40, 28], [20, 30]] and s.pool.flat.dtype == torch.uint8
        assert "MiB resident in device memory" in capsys.readouterr().out
    d = T.first_stage_stream({"class_name": "synthetic", "synthetic_of": "ddm.data.DUTSDataset"}, 2, (32, 48), CPU, 5)
    assert d.pool.n == I.ImageBatchStream.SYNTHETIC_IMAGES and (d.pool.hw_host[:, 0] > 32).any() and (d.pool.hw_host[:, 1] < 48).any()
    # the same seed draws the same pool and the same order
    e = T.first_stage_stream({"class_name": "synthetic", "synthetic_of": "ddm.data.DUTSDataset"}, 2, (32, 48), CPU, 5)
    assert torch.equal(d.pool.flat, e.pool.flat) and torch.equal(d.draw()[0], e.draw()[0])
    # SRDataset: the SR stream (its 'image' is the HR crop), real or synthetic
    sr = T.first_stage_stream({"class_name": "synthetic", "synthetic_of": "ddm.data.SRDataset"}, 2, (32, 32), CPU, 5)
    assert type(sr) is SRBatchStream and sr.channels == 3
    from PIL import Image
    (tmp_path / "hr").mkdir()
    Image.fromarray(hash_bytes((40, 44, 3), "hr0")).save(tmp_path / "hr" / "0.png")
    sr = T.first_stage_stream({"class_name": "ddm.data.SRDataset", "img_folder": str(tmp_path / "hr")}, 2, (32, 32), CPU, 5)
    assert type(sr) is SRBatchStream and sr.channels == 3 and sr.pool.n == 1
    # everything else goes to ImageStream, with its own refusals
    plain = T.first_stage_stream({"class_name": "synthetic"}, 2, (32, 32), CPU, 5)
    assert type(plain) is U.ImageStream and plain.channels == 3
    np.save(tmp_path / "ok.npy", np.zeros((3, 32, 32, 3), dtype=np.uint8))
    assert type(T.first_stage_stream({"npy": str(tmp_path / "ok.npy")}, 2, (32, 32), CPU, 5)) is U.ImageStream
    with pytest.raises(NotImplementedError, match="ddm.data.CelebAHQ"):
        T.first_stage_stream({"class_name": "ddm.data.CelebAHQ", "img_folder": "/x"}, 2, (32, 32), CPU, 5)
    with pytest.raises(NotImplementedError, match="only ddm.data.CIFAR10"):
        T.first_stage_stream({}, 2, (32, 32), CPU, 5)
    with pytest.raises(NotImplementedError, match=r"synthetic_of 'ddm.data.EdgeDataset'.*ddm.data.ImageDataset, ddm.data.DUTSDataset, "
                                                  r"ddm.data.SketchDataset and ddm.data.SRDataset"):
        T.first_stage_stream({"class_name": "synthetic", "synthetic_of": "ddm.data.EdgeDataset"}, 2, (32, 32), CPU, 5)
    for cls, key in (("ddm.data.ImageDataset", "img_folder"), ("ddm.data.DUTSDataset", "data_root"), ("ddm.data.SketchDataset", "data_root"),
                     ("ddm.data.SRDataset", "img_folder")):
        with pytest.raises(ValueError, match=f"needs data.{key}"):
            T.first_stage_stream({"class_name": cls}, 2, (32, 32), CPU, 5)
    with pytest.raises(FileNotFoundError):
        T.first_stage_stream({"class_name": "ddm.data.DUTSDataset", "data_root": str(tmp_path / "nowhere")}, 2, (32, 32), CPU, 5)
    # the unconditional drivers: ImageDataset selects the folder stream, everything else ImageStream as before
    u = U.image_stream({"class_name": "synthetic", "synthetic_of": "ddm.data.ImageDataset"}, 2, (32, 32), CPU, 5)
    assert type(u) is I.ImageFolderStream
    assert type(U.image_stream({"class_name": "synthetic"}, 2, (32, 32), CPU, 5)) is U.ImageStream
    with pytest.raises(NotImplementedError, match="only ddm.data.CIFAR10"):          # the saliency maps are no unconditional dataset
        U.image_stream({"class_name": "ddm.data.DUTSDataset", "data_root": "/x"}, 2, (32, 32), CPU, 5)


def test_channel_mismatch_errors():
    import train_vae as T
    model = lambda i, o, d=None: {"ddconfig": {"in_channels": i, "out_ch": o}, "lossconfig": ({} if d is None else {"disc_in_channels": d})}
    T.check_channels(3, model(3, 3))
    T.check_channels(1, model(1, 1, 1))
    with pytest.raises(ValueError, match="yields 1-channel images but model.ddconfig.in_channels is 3"):
        T.check_channels(1, model(3, 3))
    with pytest.raises(ValueError, match="yields 3-channel images but model.ddconfig.in_channels is 1"):
        T.check_channels(3, model(1, 1, 1))
    with pytest.raises(ValueError, match="disc_in_channels is 3 but model.ddconfig.out_ch is 1"):
        T.check_channels(1, model(1, 1))          # the default disc_in_channels is 3
    with pytest.raises(ValueError, match="disc_in_channels is 1 but model.ddconfig.out_ch is 3"):
        T.check_channels(3, model(3, 3, 1))


def test_recipe_yamls_match_the_reference_settings():
    import yaml
    import train_vae as T
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dd = lambda res, c: dict(double_z=True, z_channels=3, resolution=res, in_channels=c, out_ch=c, ch=128, ch_mult=[1, 2, 4],
                             num_res_blocks=2, attn_resolutions=[], dropout=0.0)
    want = {"saliency/duts_ae_kl_384x384.yaml": (dd([384, 384], 1), dict(disc_start=40001, kl_weight=1e-6, disc_weight=0.5, disc_in_channels=1),
                                                 "ddm.data.DUTSDataset", 8, (5e-6, 5e-7, 80000, 8000), 1),
            "sketch2img/sketchcoco_ae_kl_256x256_d4.yaml": (dd([256, 256], 3), dict(disc_start=20001, kl_weight=1e-6, disc_weight=0.5),
                                                            "ddm.data.SketchDataset", 8, (5e-6, 1e-6, 50000, 5000), 3),
            "super-resolution/div2k_ae_kl_512x512_d4.yaml": (dd([512, 512], 3), dict(disc_start=20001, kl_weight=1e-6, disc_weight=0.5),
                                                             "ddm.data.SRDataset", 4, (5e-6, 1e-6, 100000, 10000), 3)}
    for rel, (ddconfig, lossconfig, of, batch, (lr, min_lr, steps, every), ch) in want.items():
        cfg = yaml.load(open(os.path.join(root, "configs", rel)), Loader=yaml.SafeLoader)
        m, t = cfg["model"], cfg["trainer"]
        assert m["class_name"] == "ddm.encoder_decoder.AutoencoderKL" and m["embed_dim"] == 3 and m["ckpt_path"] is None, rel
        assert m["ddconfig"] == ddconfig and m["lossconfig"] == lossconfig, rel
        assert cfg["data"]["class_name"] == "synthetic" and cfg["data"]["synthetic_of"] == of and cfg["data"]["batch_size"] == batch, rel
        assert cfg["data"]["augment_horizontal_flip"] is True, rel
        assert (t["gradient_accumulate_every"], t["lr"], t["min_lr"], t["train_num_steps"], t["save_and_sample_every"]) == \
            (2, lr, min_lr, steps, every), rel
        T.check_channels(ch, m)


# ------------------------------------------------------------------------------------------------ C ABI
def test_image_resize_batch_refuses_bad_arguments_without_launching():
    """Every call has exactly one bad argument and returns ADM_EINVAL (-22).  The pointers are HOST buffers: the checks precede the
    launch, so nothing is ever read through them."""
    from adm_amd import hip
    fn = hip.lib().adm_image_resize_batch
    buf = (ctypes.c_uint32 * 256)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base)
    good = dict(pool=p, pool_bytes=64, off=p, hw=p, n_images=1, C=1, tab=p, tab_ints=64, tab_dir=p, n_tables=1, img_tab=p, max_h=32,
                max_w=32, kh=3, kv=3, idx=p, flip=p, out=p, out_u8=p, B=2, H=32, W=32)
    order = list(good)

    def rc(**bad):
        return fn(*[dict(good, **bad)[k] for k in order], None)

    for name in ("pool", "off", "hw", "tab", "tab_dir", "img_tab", "idx", "flip", "out"):          # out_u8 alone may be NULL
        assert rc(**{name: None}) == -22, name
    assert rc(pool=ctypes.c_void_p(base + 1)) == -22 and rc(pool=ctypes.c_void_p(base + 2)) == -22          # not dword-aligned
    assert rc(pool_bytes=63) == -22 and rc(pool_bytes=66) == -22 and rc(pool_bytes=0) == -22 and rc(pool_bytes=-4) == -22
    for C in (0, 2, 4, -1):
        assert rc(C=C) == -22, C
    assert rc(B=65536) == -22 and rc(B=0) == -22
    assert rc(H=65536 * 16, max_h=16, max_w=16) == -22          # 65536 rows of 16x16 tiles: grid.y
    assert hip.lib().adm_pair_resize_lds(32, 32, 32 * 9, 32 * 9, 19, 19) > 64 * 1024
    assert rc(max_h=32 * 9, max_w=32 * 9, kh=19, kv=19) == -22          # more than 64 KiB of LDS
    for name in ("n_images", "n_tables", "tab_ints", "H", "W", "max_h", "max_w", "kh", "kv"):
        assert rc(**{name: 0}) == -22, name


# ------------------------------------------------------------------------------------------------ one-channel autoencoder oracle
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "g27_ae_train_c1.npz"))


def _rel(a, b):
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _l2(a, b):
    a, b = torch.as_tensor(np.asarray(a)).double().reshape(-1), torch.as_tensor(np.asarray(b)).double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def test_golden_files_are_what_their_generators_promise(gold):
    rep = json.load(open(os.path.join(GOLDEN, "oracle_vs_reference_report_ae_train_c1.json")))
    assert len(rep["cases"]) >= 50 and all(c["ok"] and c["max_rel_err"] <= 1e-9 for c in rep["cases"])
    assert os.path.getsize(os.path.join(GOLDEN, "g27_ae_train_c1.npz")) <= os.path.getsize(os.path.join(GOLDEN, "g18_ae_train.npz"))
    assert gold["post.opt0.grad.encoder.conv_in.weight"].shape == (32, 1, 3, 3)
    assert gold["post.opt0.grad.decoder.conv_out.weight"].shape == (1, 32, 3, 3)
    assert gold["post.opt1.grad.loss.discriminator.main.0.weight"].shape == (64, 1, 4, 4)
    assert os.path.getsize(os.path.join(GOLDEN, "g28_image_data.npz")) < 200 * 1000
    g = np.load(os.path.join(GOLDEN, "g28_image_data.npz"))
    assert g["targets"].tolist() == [[32, 32], [48, 32], [40, 24]]
    assert g["c1.sizes"].tolist() == [[29, 37], [30, 38], [31, 39], [32, 40], [33, 1], [9, 11]]
    assert g["c3.sizes"].tolist() == [[20, 24], [32, 32], [103, 99], [7, 6]]
    for C in (1, 3):
        total = 0
        for i, (h, w) in enumerate(g[f"c{C}.sizes"].tolist()):
            src = g[f"c{C}.s{i}.src"]
            assert src.dtype == np.uint8 and src.shape == ((h, w, 3) if C == 3 else (h, w))
            assert np.array_equal(src, hash_bytes(src.shape, f"image_data.c{C}.s{i}"))
            total += src.size
            for H, W in g["targets"].tolist():
                out = g[f"c{C}.s{i}.t{H}x{W}"]
                assert out.shape == ((H, W, 3) if C == 3 else (H, W))
                assert np.array_equal(g[f"c{C}.s{i}.t{H}x{W}.flipped"], out[:, ::-1])
        assert total % 4 != 0          # the last image ends off a dword boundary
    assert np.array_equal(g["c3.s1.t32x32"], g["c3.s1.src"])          # the identity


@pytest.mark.parametrize("tag,idx", R1.CASES)
def test_c1_restatement_vs_golden_fp64(gold, tag, idx):
    """rtol 1e-9: both sides are fp64 torch on the CPU running the same operations (the generator measured 0 for every value)."""
    x, eps = R1.case_inputs(tag)
    assert x.shape == (2, 1, 64, 48) and eps.shape == (2, 3, 16, 12)
    loss, log, grads, sd = R1.step_with_grads(R1.case_state(tag), lpips_ref.synthetic_state_dict(), R1.LOSSCONFIG, x, eps, idx,
                                              R1.STEPS[tag])
    key = f"{tag}.opt{idx}"
    assert _rel(loss, gold[f"{key}.loss"]) <= 1e-9
    n = 0
    for k in gold.files:
        if k.startswith(f"{key}.log."):
            assert _rel(log[k[len(key) + 5:]], gold[k]) <= 1e-9, k
            n += 1
        elif k.startswith(f"{key}.grad."):
            assert _rel(grads[k[len(key) + 6:]], gold[k]) <= 1e-9, k
            n += 1
        elif k.startswith(f"{key}.bn."):
            assert _rel(sd["loss.discriminator.main.3." + k[len(key) + 4:]], gold[k]) <= 1e-9, k
    assert n == len(R1.grad_keys(tag, idx)) + (8 if idx == 0 else 3)
    if idx == 0:
        ratio = float(gold[f"{key}.log.train/d_weight"]) / R1.LOSSCONFIG["disc_weight"]
        assert 1e-3 < ratio < 1e3          # the clamp is inactive
        assert float(gold[f"{key}.log.train/disc_factor"]) == (0.0 if tag == "pre" else 1.0)
    assert int(gold[f"{key}.bn.num_batches_tracked"]) == (1 if idx == 0 else 2)


@pytest.mark.parametrize("tag", ["pre", "post"])
def test_c1_torch_fp32_deviation_on_the_same_inputs(gold, tag):
    """The yardstick of the GPU bars (tests/test_hip_ae_train_c1.py): how far plain fp32 torch lands from the fp64 golden on the
    one-channel cases.  Measured here (torch CPU): d_weight 7.0e-7 ('pre'), 1.5e-7 ('post') relative, so the GPU bar
    max(1e-3, 4 x this) is 1e-3; logs <= 3.0e-7; worst gradient 1.8e-4 / 7.9e-6 relative L2 (|x - r|, hinge, LeakyReLU, ReLU and
    max-pool kinks flip single elements), against the GPU bar of 2e-3."""
    x, eps = R1.case_inputs(tag)
    _, log, grads, _ = R1.step_with_grads(R1.case_state(tag), lpips_ref.synthetic_state_dict(), R1.LOSSCONFIG, x, eps, 0, R1.STEPS[tag],
                                          dtype=torch.float32)
    key = f"{tag}.opt0"
    dw = _rel(log["train/d_weight"], gold[f"{key}.log.train/d_weight"])
    worst = max(_l2(grads[k[len(key) + 6:]], gold[k]) for k in gold.files if k.startswith(f"{key}.grad."))
    logs = max(_rel(log[k], gold[f"{key}.log.{k}"]) for k in ("train/total_loss", "train/nll_loss", "train/kl_loss", "train/rec_loss",
                                                              "train/g_loss"))
    print(f"{tag}: fp32 torch d_weight deviation {dw:.2e}, worst gradient rel L2 {worst:.2e}, worst log {logs:.2e}")
    assert 4 * dw < 1e-3          # so the GPU test's bar max(1e-3, 4 x deviation) is 1e-3
    assert worst < 2e-3 / 4       # the gradient bar leaves room above torch's own fp32 noise
    assert logs < 1e-3 / 4
