"""CPU: the host half of the super-resolution batches (adm_amd/ddm/sr_data.py), the LR ratio of train_cond_ldm.py and the loader of
local encoder weights.  tests/golden/g21_sr_data.npz holds PIL's own bytes (tools/make_golden_sr_data.py): PIL's resize is integer
arithmetic, so every comparison is for ZERO differing bytes."""
import os

import numpy as np
import pytest
import torch

import sr_data_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_sr_data.npz")
TABLE_CASES = ("nonint", "by8", "bilinear", "tiny", "tall")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def table_resize(img, out_hw, kind):
    """The two passes with resample_table's windows and coefficients, int32 as the kernel accumulates."""
    from adm_amd.ddm.sr_data import resample_table

    def one_pass(a, n_out):
        bounds, coeffs = resample_table(a.shape[1], n_out, kind)
        assert bounds.dtype == np.int32 and coeffs.dtype == np.int32 and bounds.shape == (n_out, 2) and coeffs.shape[0] == n_out
        assert int(bounds[:, 1].max()) <= coeffs.shape[1]
        res = np.empty((a.shape[0], n_out, 3), dtype=np.uint8)
        for i, (s, n) in enumerate(bounds):
            assert not coeffs[i, n:].any()
            acc = (1 << 21) + np.tensordot(a[:, s:s + n].astype(np.int64), coeffs[i, :n].astype(np.int64), axes=([1], [0]))
            assert np.abs(acc).max() < 2 ** 31
            res[:, i] = np.clip(acc >> 22, 0, 255)
        return res

    return one_pass(one_pass(img, out_hw[1]).transpose(1, 0, 2), out_hw[0]).transpose(1, 0, 2)


def test_tables_and_restatement_reproduce_every_golden_output(g):
    n = 0
    for tag in TABLE_CASES:
        x, want, kind = g[f"{tag}.in"], g[f"{tag}.cond"], str(g[f"{tag}.kind"])
        assert np.array_equal(R.resize_u8(x, want.shape[:2], kind), want), tag
        assert np.array_equal(table_resize(x, want.shape[:2], kind), want), tag
        n += 1
    for tag in ("clipped", "edge"):
        x = g[f"{tag}.in"]
        image, cond = R.sr_pair(x, 0, 0, x.shape[:2])
        assert np.array_equal(image, g[f"{tag}.image"]) and np.array_equal(cond, g[f"{tag}.cond"]), tag
        assert np.array_equal(table_resize(x, cond.shape[:2], "bicubic"), g[f"{tag}.cond"]), tag
        n += 1
    for k, (i, t, l, f) in enumerate(g["pool.draws"]):
        image, cond = R.sr_pair(g[f"pool.in{i}"], t, l, (64, 48), flip=bool(f))
        assert np.array_equal(image, g["pool.image"][k]) and np.array_equal(cond, g["pool.cond"][k]), k
        crop = g[f"pool.in{i}"][t:t + 64, l:l + 48]
        want = table_resize(crop, (16, 12), "bicubic")
        assert np.array_equal(want[:, ::-1] if f else want, g["pool.cond"][k]), k
        n += 1
    image, cond = R.sr_test_pair(g["test.in"])
    assert cond.shape == (128, 128, 3) and np.array_equal(cond, g["test.cond"])
    pad = np.zeros((512, 512, 3), dtype=np.uint8)
    pad[:300, :260] = g["test.in"]
    assert np.array_equal(table_resize(pad, (128, 128), "bicubic"), g["test.cond"])
    assert bool(g["fliporder.equal"])          # flipping before or after the resize gave PIL the same bytes
    assert n == 10


def test_edge_case_exercises_the_uint8_intermediate(g):
    """The step-edge image: horizontal-pass values fall outside [0, 255] before the clip and the output reaches both extremes, so a
    float intermediate or a missing clip cannot reproduce it."""
    stats = {}
    cond = R.resize_u8(g["edge.in"], (8, 8), "bicubic", stats)
    assert np.array_equal(cond, g["edge.cond"])
    assert stats["horizontal_clipped"] == 116
    assert int((cond == 0).sum()) == 76 and int((cond == 255).sum()) == 85


def test_table_16_to_4_bicubic_windows():
    """support = 2 * 4 = 8, centers 2, 6, 10, 14: windows [c - 8 + .5, c + 8 + .5) truncated = [-5, 10), [-1, 14), [2, 18), [6, 22), every
    one clipped by a border of [0, 16) and renormalised (each row sums to 2^22 within the rounding of its taps)."""
    from adm_amd.ddm.sr_data import resample_table
    bounds, coeffs = resample_table(16, 4, "bicubic")
    assert bounds.tolist() == [[0, 10], [0, 14], [2, 14], [6, 10]]
    assert coeffs.shape == (4, 17)
    for i in range(4):
        n = bounds[i, 1]
        assert abs(int(coeffs[i, :n].sum()) - (1 << 22)) <= n and not coeffs[i, n:].any()
    assert np.array_equal(coeffs[0, :10], coeffs[3, :10][::-1]) and np.array_equal(coeffs[1, :14], coeffs[2, :14][::-1])
    assert coeffs[0, 0] == 826655 and coeffs[0, 6] == -54371          # hand-checked: w / sum(w) * 2^22, rounded half away from zero


def test_lanczos_and_unknown_filters_raise():
    from adm_amd.ddm.sr_data import resample_table
    with pytest.raises(NotImplementedError):
        resample_table(16, 4, "lanczos")
    with pytest.raises(ValueError):
        resample_table(16, 4, "nearest")


def test_crop_larger_than_an_image_raises():
    from adm_amd.ddm.sr_data import pack_pool
    imgs = [np.zeros((80, 72, 3), np.uint8), np.zeros((64, 47, 3), np.uint8)]
    with pytest.raises(ValueError, match="smaller than the 64x48 crop"):
        pack_pool(imgs, (64, 48))
    flat, off, hw = pack_pool(imgs, (64, 47))
    assert flat.size % 4 == 0 and flat.size >= 80 * 72 * 3 + 64 * 47 * 3 and off.tolist() == [0, 80 * 72 * 3]
    assert off.dtype == np.int64 and hw.tolist() == [[80, 72], [64, 47]]


def test_lr_ratio_of_the_conditional_trainer():
    from adm_amd.optim import lr_lambda_cond
    lr, min_lr, N = 5e-5, 5e-6, 400000
    assert lr_lambda_cond(0, lr, min_lr, N) == 1.0
    for it in (1, 123456, 300000):
        assert lr_lambda_cond(it, lr, min_lr, N) == max((1 - it / N) ** 0.96, min_lr / lr)
    assert lr_lambda_cond(1, lr, min_lr, N) < 1.0          # no warm-up: the decay starts at once
    assert lr_lambda_cond(399999, lr, min_lr, N) == min_lr / lr
    for it in (N, N + 1, 2 * N):
        assert lr_lambda_cond(it, lr, min_lr, N) == min_lr / lr


def _small_swin():
    from adm_amd.unet.swin_transformer import SwinTransformer
    return SwinTransformer(patch_size=[4, 4], embed_dim=32, depths=[1, 1, 2, 1], num_heads=[1, 2, 4, 8], window_size=[7, 7],
                           num_classes=10)


def test_encoder_weights_loader(tmp_path):
    from adm_amd.unet.swin_transformer import load_encoder_weights
    torch.manual_seed(3)
    src = _small_swin()
    with torch.no_grad():
        for p in src.parameters():
            p.copy_(torch.randn_like(p))
    own = {k: v.clone() for k, v in src.state_dict().items()}
    # torchvision's naming: the patch embedding is features.0, everything else moves up by one
    tv = {}
    for k, v in own.items():
        parts = k.split(".")
        if parts[0] == "first_coonv":
            tv[".".join(["features", "0"] + parts[1:])] = v
        elif parts[0] == "features":
            tv[".".join(["features", str(int(parts[1]) + 1)] + parts[2:])] = v
        else:
            tv[k] = v
    assert "features.0.0.weight" in tv and "features.7.0.norm1.weight" in tv
    for name, sd in (("tv.pth", tv), ("own.pth", own)):
        torch.save(sd, tmp_path / name)
        enc = _small_swin()
        assert load_encoder_weights(enc, str(tmp_path / name)) == []
        got = enc.state_dict()
        assert all(torch.equal(got[k], own[k]) for k in own), name
    # head.* (and norm.*, first_coonv.*) may be absent
    part = {k: v for k, v in own.items() if k.startswith("features.")}
    torch.save(part, tmp_path / "part.pth")
    enc = _small_swin()
    before = {k: v.clone() for k, v in enc.state_dict().items()}
    absent = load_encoder_weights(enc, str(tmp_path / "part.pth"))
    assert absent and all(k.split(".")[0] in ("first_coonv", "norm", "head") for k in absent)
    got = enc.state_dict()
    assert all(torch.equal(got[k], own[k]) for k in part) and all(torch.equal(got[k], before[k]) for k in absent)
    # a missing features.* tensor raises, under either naming; so does a tensor of another shape
    for sd, drop in ((own, "features.2.0.attn.qkv.weight"), (tv, "features.3.0.attn.qkv.weight")):
        torch.save({k: v for k, v in sd.items() if k != drop}, tmp_path / "lost.pth")
        with pytest.raises(RuntimeError, match="lacks 1 of the encoder's features"):
            load_encoder_weights(_small_swin(), str(tmp_path / "lost.pth"))
    bad = dict(own)
    bad["features.0.0.mlp.0.weight"] = torch.zeros(3, 3)
    torch.save(bad, tmp_path / "bad.pth")
    with pytest.raises(RuntimeError, match="features.0.0.mlp.0.weight"):
        load_encoder_weights(_small_swin(), str(tmp_path / "bad.pth"))
