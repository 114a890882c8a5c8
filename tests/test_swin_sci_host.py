"""CPU: the single-channel Swin condition encoder and the sketch-to-image recipe without a GPU -- the module tree and state-dict
shapes of ``in_chans=1``, the loader's mean over a 3-channel ImageNet stem, the import alias, the wiring of ``single_channel_cond``
into the two denoiser classes, the two YAMLs, the file discovery of ``ddm.data.SketchDataset``, the restatement
tests/swin_sci_ref.py against the float64 outputs the reference's own classes gave (tests/golden/g25_swin_sci.npz, written by
tools/make_golden_swin_sci.py), and the new entry points in the header and the binding."""
import importlib
import json
import os
import re

import numpy as np
import pytest
import torch
import yaml

import swin_ref as R
import swin_sci_ref as C
import swin_train_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


def _small(**kw):
    from adm_amd.unet.swin_transformer import SwinTransformer
    return SwinTransformer(patch_size=[4, 4], embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=[7, 7], **kw)


def test_constructor_and_state_dict_shapes(golden):
    from adm_amd.unet.swin_transformer import swin_b
    for tag, m in (("small", _small(in_chans=1)), ("swin_b", swin_b(in_chans=1))):
        want = json.loads(str(golden[f"{tag}.keys"]))          # the reference's own state_dict of swin_transformer_for_sci
        got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert got == want, [a for a, b in zip(got, want) if a != b][:5]
        assert m.in_chans == 1 and m.first_coonv[0].in_channels == 1 and all(not p.requires_grad for p in m.parameters())
    assert tuple(swin_b(in_chans=1).state_dict()["first_coonv.0.weight"].shape) == (128, 1, 4, 4)
    three, one = _small(), _small(in_chans=1)
    assert three.in_chans == 3 and tuple(three.first_coonv[0].weight.shape) == (32, 3, 4, 4)          # the default is unchanged
    assert [k for k in three.state_dict()] == [k for k in one.state_dict()]
    for bad in (2, 4, 0):
        with pytest.raises(NotImplementedError, match="in_chans"):
            _small(in_chans=bad)
    m = _small(in_chans=1)
    with pytest.raises(RuntimeError, match="with 1 channels"):
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="with 3 channels"):
        _small()(torch.zeros(1, 1, 32, 32))


def test_loader_averages_a_three_channel_stem(tmp_path):
    from adm_amd.unet.swin_transformer import load_encoder_weights
    sd3 = R.cast(R.filled_state_dict(**R.SMALL), torch.float32)
    # torchvision's naming: the patch embedding is features.0, the stages features.1 ...
    tv = {}
    for k, v in sd3.items():
        parts = k.split(".")
        if parts[0] == "first_coonv":
            k = ".".join(["features", "0"] + parts[1:])
        elif parts[0] == "features":
            k = ".".join(["features", str(int(parts[1]) + 1)] + parts[2:])
        tv[k] = v
    path3, path1 = str(tmp_path / "tv3.pth"), str(tmp_path / "own1.pth")
    torch.save(tv, path3)
    m = _small(in_chans=1)
    assert load_encoder_weights(m, path3) == []
    want = sd3["first_coonv.0.weight"].mean(dim=1, keepdim=True)
    assert tuple(m.first_coonv[0].weight.shape) == (32, 1, 4, 4) and torch.equal(m.first_coonv[0].weight, want)
    assert torch.equal(m.first_coonv[0].bias, sd3["first_coonv.0.bias"])
    assert torch.equal(m.features[0][0].attn.qkv.weight, sd3["features.0.0.attn.qkv.weight"])
    # a one-channel stem loads as it is (the encoder's own naming)
    sd1 = R.cast(C.filled_state_dict(**R.SMALL), torch.float32)
    torch.save(sd1, path1)
    m = _small(in_chans=1)
    load_encoder_weights(m, path1)
    assert torch.equal(m.first_coonv[0].weight, sd1["first_coonv.0.weight"])
    # the 3-channel encoder's rules are unchanged: it keeps the 3-channel stem and refuses a 1-channel one
    m3 = _small()
    load_encoder_weights(m3, path3)
    assert torch.equal(m3.first_coonv[0].weight, sd3["first_coonv.0.weight"])
    with pytest.raises(RuntimeError, match="first_coonv.0.weight"):
        load_encoder_weights(_small(), path1)


def test_import_alias():
    A = importlib.import_module("unet.swin_transformer_for_sci")
    B = importlib.import_module("adm_amd.unet.swin_transformer_for_sci")
    from adm_amd.unet.swin_transformer import SwinTransformer
    assert A.swin_b is B.swin_b and A.SwinTransformer is SwinTransformer
    m = A.swin_b()
    assert isinstance(m, SwinTransformer) and m.in_chans == 1
    with pytest.raises(TypeError):
        A.swin_b(weights=None)


def _unet(U, **kw):
    return U.Unet(dim=32, dim_mults=(1, 2, 4, 8), cond_dim=32, cond_dim_mults=(), channels=3, cond_in_dim=1,
                  window_sizes1=[[8, 8], [4, 4], [2, 2], [1, 1]], window_sizes2=[[8, 8], [4, 4], [2, 2], [1, 1]], fourier_scale=16, **kw)


def test_unet_wiring():
    import adm_amd.unet.cond_unet as U2
    import adm_amd.unet.cond_unet_sd as U1
    from adm_amd.unet.swin_transformer import SwinTransformer
    for kw in (dict(cfg={"cond_net": "swin"}, single_channel_cond=True), dict(cfg={"cond_net": "swin", "single_channel_cond": True})):
        m = _unet(U2, cond_encoder="swin_b", **kw)
        assert isinstance(m.init_conv_mask, SwinTransformer) and m.init_conv_mask.in_chans == 1
        assert tuple(m.state_dict()["init_conv_mask.first_coonv.0.weight"].shape) == (128, 1, 4, 4)
    assert _unet(U2, cond_encoder="swin_b", cfg={"cond_net": "swin"}).init_conv_mask.in_chans == 3
    m = _unet(U2, cond_encoder="swin_b", cfg={"cond_net": "swin"}, single_channel_cond=True, train_cond_encoder=True)
    assert m.init_conv_mask.trainable and m.init_conv_mask.first_coonv[0].weight.requires_grad
    with pytest.raises(NotImplementedError, match="single_channel_cond"):
        _unet(U1, cond_encoder="swin_b", cfg={"cond_net": "swin"}, single_channel_cond=True)


def test_committed_yamls_carry_the_recipe():
    def resolve(path):
        mod, _, attr = path.rpartition(".")
        return getattr(importlib.import_module(mod), attr)

    for name, sample in (("sketchcoco_cond_ddm_const_ldm.yaml", False), ("sketchcoco_cond_ddm_const_ldm_sample.yaml", True)):
        text = open(os.path.join(ROOT, "configs", "sketch2img", name)).read()
        cfg = yaml.load(text, Loader=yaml.SafeLoader)
        m, u, fs, d, t = cfg["model"], cfg["model"]["unet"], cfg["model"]["first_stage"], cfg["data"], cfg["trainer"]
        for cls in (m["class_name"], u["class_name"], fs["class_name"]):
            assert isinstance(resolve(cls), type), cls
        assert m["class_name"] == "ddm.ddm_const.LatentDiffusion" and m["image_size"] == [256, 256] and m["sampling_timesteps"] == 10
        assert m["use_l1"] is True and m["weighting_loss"] is False and m["scale_factor"] == 0.125 and m["scale_by_std"] is True
        assert "use_disloss" not in m and "use_disloss" in text.split("\nmodel:")[0]          # left out, and the header says why
        dd = fs["ddconfig"]
        assert (dd["in_channels"], dd["out_ch"], dd["ch"], dd["ch_mult"], dd["z_channels"]) == (3, 3, 128, [1, 2, 4], 3)
        assert dd["resolution"] == [256, 256] and fs["lossconfig"]["disc_start"] == 20001 and not fs["ckpt_path"]
        assert u["class_name"] == "unet.cond_unet.Unet" and u["single_channel_cond"] is True and u["cond_in_dim"] == 1
        assert u["dim"] == 128 and u["dim_mults"] == [1, 2, 4, 4] and u["channels"] == 3 and u["cond_feature_size"] == [128, 128]
        assert u["fix_bb"] is False and u["cond_encoder"] == "swin_b" and u["train_cond_encoder"] is True
        assert d["image_size"] == [256, 256] and not d["data_root"]
        assert (t["gradient_accumulate_every"], t["lr"], t["min_lr"], t["train_num_steps"]) == (2, 5e-5, 5e-6, 300000)
        assert t["ema_update_after_step"] == 20000 and t["ema_update_every"] == 8 and not os.path.isabs(t["results_folder"])
        if sample:
            s = cfg["sampler"]
            assert d["class_name"] == "synthetic" and d["synthetic_of"] == "ddm.data.SketchDataset"
            assert d["split"] == "test" and d["augment_horizontal_flip"] is False
            assert s["out_channels"] == 3 and s["crop_size"] == s["stride"] == [256, 256] and s["cond_encoder"] == "swin_b"
            assert not os.path.isabs(s["ckpt_path"]) and not os.path.isabs(s["save_folder"])
        else:
            assert d["class_name"] == "synthetic" and d["synthetic_of"] == "ddm.data.SketchDataset" and d["split"] == "train"
            assert d["batch_size"] == 16 and d["augment_horizontal_flip"] is True


def _tree(root, split, names):
    from PIL import Image
    for sub, name, psz, ssz in names:
        for kind, size, mode in (("GT", psz, "RGB"), ("Sketch", ssz, "L")):
            folder = root / kind / split / sub
            folder.mkdir(parents=True, exist_ok=True)
            Image.new(mode, (size[1], size[0]), 7).save(folder / name)


def test_find_sketch_pairs_and_missing_sketch(tmp_path):
    from adm_amd.ddm.pair_data import SKETCH_CLASSES, DUTSBatchStream, SketchBatchStream, find_sketch_pairs, load_sketch
    from train_cond_ldm import batch_stream
    assert SKETCH_CLASSES == ("ddm.data.SketchDataset", "SketchDataset")
    _tree(tmp_path, "train", [("cat", "b.png", (20, 24), (20, 24)), ("cat", "a.png", (16, 18), (32, 36)), ("dog", "c.png", (24, 20), (24, 20))])
    _tree(tmp_path, "val", [("cat", "v.png", (20, 24), (10, 12))])
    (tmp_path / "GT" / "train" / "cat" / "._a.png").write_bytes(b"resource fork")          # skipped by name (data.py:1050)
    (tmp_path / "GT" / "train" / "cat" / "notes.jpg").write_bytes(b"not a png")
    pairs = find_sketch_pairs(str(tmp_path), "train")
    assert [(p.relative_to(tmp_path).as_posix(), s.relative_to(tmp_path).as_posix()) for p, s in pairs] == [
        ("GT/train/cat/a.png", "Sketch/train/cat/a.png"), ("GT/train/cat/b.png", "Sketch/train/cat/b.png"),
        ("GT/train/dog/c.png", "Sketch/train/dog/c.png")]
    assert [p.name for p, _ in find_sketch_pairs(str(tmp_path), "test")] == ["v.png"]          # split: test reads val
    # the reference's own rule for a bare folder gives the same sketch
    bare = find_sketch_pairs(str(tmp_path / "GT" / "train"), "all")
    assert [s for _, s in bare] == [s for _, s in pairs]
    photos, sketches, names = load_sketch(str(tmp_path), "train")
    assert names == ["a.png", "b.png", "c.png"] and photos[0].shape == (16, 18, 3) and sketches[0].shape == (32, 36)
    assert photos[0].dtype == np.uint8 and sketches[0].dtype == np.uint8 and sketches[0].ndim == 2
    # the stream by class name, and the roles
    for cfg in ({"class_name": "ddm.data.SketchDataset", "data_root": str(tmp_path)}, {"class_name": "SketchDataset", "data_root": str(tmp_path)},
                {"class_name": "synthetic", "synthetic_of": "ddm.data.SketchDataset"}):
        s = batch_stream(cfg, 2, (16, 24), CPU, 1)
        assert type(s) is SketchBatchStream and s.ROLES == ("image", "cond") and s.pool.out_hw == (16, 24), cfg
    assert DUTSBatchStream.ROLES == ("cond", "image") and issubclass(DUTSBatchStream, type(s).__mro__[1])          # one shared base
    with pytest.raises(ValueError, match="data_root"):
        batch_stream({"class_name": "ddm.data.SketchDataset"}, 2, (16, 24), CPU, 1)
    # a missing sketch raises at start-up and names the file
    (tmp_path / "Sketch" / "train" / "dog" / "c.png").unlink()
    with pytest.raises(FileNotFoundError, match=re.escape(os.path.join("Sketch", "train", "dog", "c.png"))):
        find_sketch_pairs(str(tmp_path), "train")
    # an unreadable one too
    (tmp_path / "Sketch" / "train" / "dog" / "c.png").write_bytes(b"not an image")
    with pytest.raises(OSError, match="c.png"):
        load_sketch(str(tmp_path), "train")


def _same(got, want, rtol=1e-12, atol=1e-13):
    np.testing.assert_allclose(got.numpy(), want, rtol=rtol, atol=atol)


@pytest.mark.parametrize("name", list(C.STEM_CASES))
def test_ref_stem_reproduces_golden(golden, name):
    B, H, W, E = C.STEM_CASES[name]
    sd = C.stem_params(E)
    for content in C.STEM_CONTENTS:
        y = C.stem(sd, C.stem_input(name, content))
        assert tuple(y.shape) == (B, H // 4, W // 4, E)
        _same(R.sample(y), golden[f"stem.{name}.{content}"], atol=1e-11)          # (+300: conv outputs of ~1e2 before the norm)


@pytest.mark.parametrize("name,cfg,shape", [("small", R.SMALL, C.SMALL_INPUT), ("b64", R.SWIN_B, C.SWIN_B_INPUT)])
def test_ref_model_reproduces_golden(golden, name, cfg, shape):
    sd = C.filled_state_dict(**cfg)
    assert tuple(sd["first_coonv.0.weight"].shape) == (cfg["embed_dim"], 1, 4, 4)
    ys = C.forward(sd, C.model_input(name, shape), cfg["depths"], cfg["num_heads"])
    assert [list(y.shape) for y in ys] == golden[f"{name}.shapes"].tolist()
    for i, y in enumerate(ys):
        _same(R.sample(y), golden[f"{name}.stage{i}"])


@pytest.mark.parametrize("tag,p,keep", C.TRAIN_TAGS, ids=[t[0] for t in C.TRAIN_TAGS])
def test_ref_stem_gradients_reproduce_golden(golden, tag, p, keep):
    for k, g in C.stem_grads(R.SMALL, C.SMALL_INPUT, "small", tag, keep, p).items():
        _same(T.sample_grad(g), golden[f"{tag}.{k}"], rtol=1e-10, atol=1e-12 * float(g.abs().max()))


def test_new_symbols_are_declared_and_bound():
    from adm_amd import hip, ops_swin
    header = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    for name in ("adm_patch_embed_ln_fwd", "adm_patch_embed_ln_bwd", "adm_patch_embed_ln_bwd_ws_floats"):
        assert re.search(rf"\b{name}\(", header), name
        assert name in hip.EXPORTS and hasattr(hip.lib(), name)
    assert "adm_patch_embed_ln_bwd_ws_floats" in hip.NO_STREAM
    lib = hip.lib()
    assert lib.adm_patch_embed_ln_bwd_ws_floats(16, 256, 256, 128) == 256 * 19 * 128          # one partial per workgroup, at most 256
    assert lib.adm_patch_embed_ln_bwd_ws_floats(1, 4, 4, 32) == 19 * 32
    assert lib.adm_patch_embed_ln_bwd_ws_floats(1, 3, 8, 32) == 0 and lib.adm_patch_embed_ln_bwd_ws_floats(1, 8, 8, 48) == 0
    assert callable(ops_swin.patch_embed_ln)
    with pytest.raises(RuntimeError, match="no gradient for its input"):
        ops_swin.patch_embed_ln(torch.zeros(1, 1, 8, 8, requires_grad=True), torch.zeros(32, 1, 4, 4), *(torch.zeros(32),) * 3)
