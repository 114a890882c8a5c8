"""CPU: the host half of the restoration score (adm_amd/metrics/restoration.py) against the per-image restatement
(tests/restoration_ref.py), the golden file, the C ABI's declaration and refusals, the opt-in sampler key and eval_restoration.py's
refusals.

Bar: per-plane SSIM within 1e-10 absolute (R.BAR; tests/test_hip_restoration_metrics.py derives it).  The restatement's direct 2-D
window against scipy's convolve2d and against the separable float64 order of the kernel is the same quantity, measured at most 2.5e-12
(flat 255 / 254, where the variance terms cancel at magnitude 65025); a float32 copy of the separable filter is 6.7e-5 off there, and
the bar must say so.
"""
import ctypes
import glob
import json
import math
import os
import re

import numpy as np
import pytest

import restoration_ref as R
from adm_amd.metrics import restoration as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden():
    g = np.load(R.GOLDEN)
    tags = sorted({k.rsplit(".", 1)[0] for k in g.files})
    return g, tags


def parse(tag):
    family, shape, c, s = tag.rsplit("_", 3)
    return family, tuple(int(v) for v in shape.split("x")), int(c[1:]), int(s[1:])


def test_restatement_equals_scipy_convolve2d_on_the_golden_pairs():
    g, tags = golden()
    report = json.load(open(R.REPORT))
    assert os.path.getsize(R.GOLDEN) < 64 * 1024 and len(tags) >= 8 and sorted(report) == tags
    assert {parse(t)[0] for t in tags} == set(R.FAMILIES) and {parse(t)[2] for t in tags} == {1, 3} and {parse(t)[3] for t in tags} == {0, 4}
    worst = 0.0
    for tag in tags:
        family, shape, C, s = parse(tag)
        p, t = g[f"{tag}.pred"], g[f"{tag}.target"]
        assert np.array_equal(p, R.case(family, shape, C)[0]) and np.array_equal(t, R.case(family, shape, C)[1])
        direct, scipy_form, separable = (R.image_ref(p, t, s, ssim=f) for f in (R.ssim_map, R.ssim_scipy, R.ssim_separable))
        for other in (scipy_form, separable):
            gap = float(np.abs(other["ssim_planes"] - direct["ssim_planes"]).max())
            worst = max(worst, gap)
            assert gap <= R.BAR, (tag, gap)
            assert other["sse"] == direct["sse"]
        assert report[tag]["vs_scipy_convolve2d"] <= R.BAR and report[tag]["vs_separable_float64"] <= R.BAR
        assert report[tag]["sse"] == [str(v) for v in direct["sse"]]
    print(f"worst direct-window distance from scipy / separable float64: {worst:.3g}")


def test_host_half_reproduces_the_golden_metrics_from_the_golden_sums():
    g, tags = golden()
    for tag in tags:
        family, shape, C, s = parse(tag)
        hw = (shape[0] - 2 * s, shape[1] - 2 * s)
        got = M.per_image(g[f"{tag}.sse"][None], g[f"{tag}.ssim_sum"][None], hw)
        keys = M.KEYS if C == 3 else M.KEYS[:2]
        assert set(got) == set(keys) | {"ssim_planes", "sse_planes"}
        want = R.image_ref(g[f"{tag}.pred"], g[f"{tag}.target"], s)
        assert list(got["sse_planes"][0]) == want["sse"]
        for k, v in zip(keys, g[f"{tag}.values"]):
            assert got[k][0] == v == want[k] or abs(got[k][0] - v) <= 1e-12 >= abs(v - want[k]), (tag, k, got[k][0], v, want[k])
        assert np.abs(got["ssim_planes"][0] - want["ssim_planes"]).max() <= 1e-15
        if family == "equal":
            assert got["psnr"][0] == math.inf and got["ssim"][0] == 1.0 and got["psnr_y"][0] == math.inf and got["ssim_y"][0] == 1.0
        one = M.metrics_from_sums(g[f"{tag}.sse"][None], g[f"{tag}.ssim_sum"][None], hw)
        assert one["images"] == 1 and all(one[k] == got[k][0] for k in keys)


def test_two_word_sse_is_reassembled_with_python_integers():
    """A synthetic sum above 2^63 (no image): 2^24 pixels of the largest Y difference, (255 x 219000)^2 each."""
    n = 1 << 24
    d2 = (255 * 219000) ** 2
    big = n * d2
    assert big > 1 << 63
    rgb = [n * 255 * 255] * 3
    sse = R.words(rgb + [big])
    assert int(sse[3, 1]) > (1 << 31) and 0 <= int(sse[3, 0]) < (1 << 32)          # hi alone passes 32 bits' worth of int64 range
    got = M.per_image(sse[None], np.zeros((1, 4)), (4096, 4096))
    assert list(got["sse_planes"][0]) == rgb + [big]
    # every pixel at the largest difference: MSE = 255^2 on RGB, 219^2 on Y
    assert got["psnr"][0] == 0.0 and got["psnr_y"][0] == pytest.approx(10 * math.log10(255 ** 2 / 219 ** 2), abs=1e-12)
    # the words are {lo, hi}, not two halves of an int64: lo at its ceiling, hi = 0
    assert M.per_image(np.array([[[(1 << 32) - 1, 0]]]), np.zeros((1, 1)), (11, 11))["sse_planes"][0, 0] == (1 << 32) - 1
    with pytest.raises(ValueError, match="SSE words"):
        M.per_image(np.array([[[1 << 32, 0]]]), np.zeros((1, 1)), (11, 11))
    # SSE = 0 is inf, kept; a data set with one such image has an infinite mean
    two = M.metrics_from_sums(np.array([[[0, 0]], [[121, 0]]]), np.full((2, 1), 1.0), (11, 11))
    assert two["psnr"] == math.inf and two["ssim"] == 1.0 and two["images"] == 2 and set(two) == {"psnr", "ssim", "images"}
    empty = M.metrics_from_sums(np.zeros((0, 4, 2), np.int64), np.zeros((0, 4)), (11, 11))
    assert empty["images"] == 0 and all(math.isnan(empty[k]) for k in M.KEYS)
    with pytest.raises(ValueError, match="smaller than the 11x11 window"):
        M.per_image(np.zeros((1, 1, 2), np.int64), np.zeros((1, 1)), (10, 30))


def test_the_bar_rejects_a_float32_filter():
    """The defect the bar is there for: the separable filter in float32 on flat 255 against flat 254 is 6.7e-5 off (w*x^2 - mu^2 cancels
    at magnitude 65025 against C2 = 58.5); the same filter in float64 passes."""
    p, t = R.case("flat", (24, 24), 1)
    direct = R.ssim_map(p[0].astype(np.float64), t[0].astype(np.float64)).mean()
    f32 = float(R.ssim_separable(p[0], t[0], np.float32).astype(np.float64).mean())
    f64 = float(R.ssim_separable(p[0], t[0], np.float64).mean())
    print(f"flat 255 / 254: float32 separable off by {abs(f32 - direct):.3g}, float64 separable by {abs(f64 - direct):.3g}")
    assert abs(f32 - direct) > 1e4 * R.BAR
    assert abs(f64 - direct) <= R.BAR
    report = json.load(open(R.REPORT))
    assert report["flat_24x24_c3_s0"]["vs_separable_float32"] > 1e4 * R.BAR


def test_definitions_known_answers():
    # Y of white is 235, of black 16: the unrounded BT.601 studio range
    white, black = np.full((3, 11, 11), 255, np.uint8), np.zeros((3, 11, 11), np.uint8)
    assert R.planes(white)[0][3, 0, 0] == 235.0 and R.planes(black)[0][3, 0, 0] == 16.0
    r = R.image_ref(white, black)
    assert r["psnr"] == 0.0 and r["psnr_y"] == pytest.approx(10 * math.log10(255 ** 2 / 219 ** 2), abs=1e-12)
    assert r["ssim"] == pytest.approx(R.C1 / (255 ** 2 + R.C1), abs=1e-12)
    w = R.window1d()
    assert len(w) == 11 and abs(w.sum() - 1) < 1e-15 and np.array_equal(w, w[::-1]) and abs(R.window2d().sum() - 1) < 1e-15
    # the shave is addressing only: scoring a shaved pair equals scoring the cut arrays
    p, t = R.case("noise", (27, 25), 3)
    a, b = R.image_ref(p, t, 4), R.image_ref(np.ascontiguousarray(p[:, 4:-4, 4:-4]), np.ascontiguousarray(t[:, 4:-4, 4:-4]), 0)
    assert a["sse"] == b["sse"] and np.array_equal(a["ssim_planes"], b["ssim_planes"])
    # the quantiser: ties to even, clamps, NaN -> 0
    assert R.quantise(np.float32([-1, 0, 0.5, 1, 7, np.nan, np.inf, -np.inf])).tolist() == [0, 0, 128, 255, 255, 0, 255, 0]          # 127.5 -> 128


def test_entry_points_are_declared_bound_and_refuse_before_launching():
    from adm_amd import hip
    header = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    for name, n in (("adm_restoration_sums", 14), ("adm_restoration_blocks", 2)):
        decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.M | re.S)
        assert decl and len(decl.group(1).split(",")) == n == len(hip._SIGS[name]), name
        assert name in hip.EXPORTS
    assert "adm_restoration_sums" not in hip.NO_STREAM and "adm_restoration_blocks" in hip.NO_STREAM
    assert f"#define ADM_RESTORATION_WINDOW {M.WINDOW}" in header and "#define ADM_RESTORATION_MAX_PIXELS (1L << 24)" in header
    tile = int(re.search(r"#define ADM_RESTORATION_TILE (\d+)", header).group(1))
    assert "restoration_metrics.hip" in open(os.path.join(ROOT, "adm_amd", "csrc", "Makefile")).read()
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = hip.lib()
    blocks = lib.adm_restoration_blocks
    assert blocks(11, 11) == 1 and blocks(tile + 10, tile + 10) == 1 and blocks(tile + 11, tile + 10) == 2 and blocks(tile + 11, 2 * tile + 11) == 6
    assert blocks(10, 11) == -22 and blocks(11, 10) == -22 and blocks(0, 0) == -22
    fn = lib.adm_restoration_sums
    a = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused before a launch
    ok = dict(pred=a, pf=0, target=a, tf=0, sse=a, ssim=a, partial=a, ticket=a, B=1, C=3, H=32, W=32, s=4)
    call = lambda **kw: fn(*{**ok, **kw}.values(), None)
    odd = ctypes.c_void_p(4098)
    for bad in (dict(pred=None), dict(target=None), dict(sse=None), dict(ssim=None), dict(partial=None), dict(ticket=None), dict(B=0),
                dict(B=65536), dict(C=2), dict(C=0), dict(C=4), dict(s=-1), dict(H=18, s=4), dict(W=18, s=4), dict(H=10, s=0), dict(H=0),
                dict(H=4097, W=4096, s=0), dict(H=11, W=(1 << 24) // 11 + 1, s=0), dict(s=1 << 30), dict(pred=odd, pf=1),
                dict(target=odd, tf=1), dict(sse=odd), dict(ssim=odd), dict(partial=odd), dict(ticket=odd)):
        assert call(**bad) == -22, bad


def test_sampler_key_is_opt_in_and_raises_by_name_elsewhere():
    import sample_cond_ldm
    from adm_amd.ddm import datasets
    assert datasets.Sampling._fields == ("form", "item", "split_test", "no_flip", "one_window", "psnr", "gray", "save_masks", "synthetic",
                                         "depth", "saliency")          # no field was added for this score
    scorer = sample_cond_ldm.restoration_scorer
    sr, inpaint = {"class_name": "ddm.data.SRDatasetTest"}, {"class_name": "ddm.data.InpaintDataset"}
    for cfg in (sr, inpaint, {"class_name": "synthetic"}, {}):
        assert scorer(cfg, {}) is None and scorer(cfg, {"cal_restoration": False}) is None
    for cfg, border in ((sr, 4), ({"class_name": "synthetic"}, 4), ({"class_name": "synthetic", "synthetic_of": "ddm.data.InpaintDataset"}, 4),
                        (inpaint, 0)):          # (synthetic_of in-painting falls through to the SR items at sampling time)
        score = scorer(cfg, {"cal_restoration": True})
        assert isinstance(score, M.RestorationScore) and score.crop_border == border, cfg
        assert scorer(cfg, {"cal_restoration": True, "restoration_crop_border": 2}).crop_border == 2
        assert scorer(cfg, {"cal_restoration": True, "restoration_crop_border": 0}).crop_border == 0
    for other in ({"class_name": "ddm.data.DUTSDataset", "split": "test"}, {"class_name": "ddm.data.SketchDataset", "split": "test"},
                  {"class_name": "ddm.data.NYUDv2DepthDataset", "split": "test"}, {"class_name": "synthetic", "synthetic_of": "ddm.data.SketchDataset"},
                  {"class_name": "synthetic", "synthetic_of": "ddm.data.NYUDv2DepthDataset"}):
        with pytest.raises(ValueError, match=r"sampler.cal_restoration: True scores restored photographs, but data.class_name '" + other["class_name"]):
            scorer(other, {"cal_restoration": True})
        assert scorer(other, {}) is None
    for path in glob.glob(os.path.join(ROOT, "configs", "**", "*.yaml"), recursive=True):
        assert "cal_restoration" not in open(path).read(), path


def test_wrapper_refuses_a_cpu_tensor():
    import torch
    z = torch.zeros(1, 3, 16, 16, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="the prediction is on cpu"):
        M.restoration_sums(z, z)


def test_eval_restoration_refuses_by_file_name(tmp_path):
    from PIL import Image
    import eval_restoration
    pred, target = tmp_path / "pred", tmp_path / "target"
    pred.mkdir(), target.mkdir()
    rng = np.random.default_rng(3)
    img = lambda h, w: Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8))
    img(20, 24).save(target / "a.png"), img(20, 24).save(target / "b.png")
    img(20, 24).save(pred / "a.png")
    args = ["--pred", str(pred), "--target", str(target)]
    with pytest.raises(FileNotFoundError, match=r"the prediction for .*target.b\.png is missing"):
        eval_restoration.main(args)
    img(20, 23).save(pred / "b.jpg")          # paired by stem, whatever the extension
    with pytest.raises(ValueError, match=r"pred.b\.jpg is 20x23 but its target .*b\.png is 20x24: nothing is resized"):
        eval_restoration.main(args)
    os.remove(pred / "b.jpg")
    img(20, 24).save(pred / "b.png")
    with pytest.raises(ValueError, match=r"pred.a\.png is 20x24: shaved by --crop-border 5 it leaves 10x14"):
        eval_restoration.main(args + ["--crop-border", "5"])
    with pytest.raises(FileNotFoundError):
        eval_restoration.main(["--pred", str(pred), "--target", str(tmp_path / "nowhere")])
