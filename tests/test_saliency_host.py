"""CPU: the host half of the saliency score (adm_amd/metrics/saliency.py) against the per-pixel restatement (tests/saliency_ref.py), its
known answers, the data-set reduction, the golden file, the C ABI's declaration and refusals, the dataset table and the opt-in key.

Bar: 1e-12 absolute.  Both routes -- integer tables, and one mask per threshold -- end in fewer than a hundred float64 roundings on
values of order 1 after exact integer sums (the per-pixel float sums are pairwise, over at most 2145 terms of order 1); measured 4.4e-16.
"""
import ctypes
import glob
import inspect
import json
import os
import re

import numpy as np
import pytest

import saliency_ref as R
from adm_amd.metrics import saliency as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-12


def from_pair(p, m, normalize=True):
    tables, head = R.tables_ref(p, m)
    return {k: v[0] for k, v in S.per_image(tables[None], head[None], p.shape, normalize).items()}


@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "raw"])
@pytest.mark.parametrize("shape", R.HOST_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_tables_route_equals_the_per_pixel_restatement(family, shape, normalize):
    p, m = R.case(family, shape)
    got, want = from_pair(p, m, normalize), R.image_ref(p, m, normalize)
    assert set(got) == set(want)
    for k in want:
        gap = float(np.abs(got[k] - want[k]).max())
        assert gap <= BAR, (k, gap)
        assert np.isfinite(got[k]).all()
    one = S.metrics_from_tables(*[a[None] for a in R.tables_ref(p, m)], shape, normalize)
    ref = R.dataset_ref([(p, m)], normalize)
    assert one["images"] == 1 and all(abs(one[k] - ref[k]) <= BAR for k in S.KEYS)


@pytest.mark.parametrize("shape", [(7, 13), (33, 65)], ids=lambda s: "%dx%d" % s)
def test_known_answers(shape):
    n = shape[0] * shape[1]
    p, m = R.case("perfect", shape)
    r = from_pair(p, m)
    assert r["mae"] == 0.0 and abs(r["s_measure"] - 1.0) <= BAR
    assert np.abs(r["f_curve"][1:] - 1.0).max() <= BAR          # k = 0 switches every pixel on
    assert np.abs(r["e_curve"][1:] - n / (n - 1)).max() <= BAR          # the definition's quirk, kept
    assert abs(r["adp_f"] - 1.0) <= BAR and abs(r["adp_e"] - n / (n - 1)) <= BAR
    p, m = R.case("inverted", shape)
    r = from_pair(p, m)
    assert r["mae"] == 1.0 and r["s_measure"] == 0.0
    # a constant prediction is not stretched: its value stays 77 / 255
    p, m = R.case("constant", shape)
    n_f = int((m > 128).sum())
    for normalize in (True, False):
        r = from_pair(p, m, normalize)
        assert abs(r["mae"] - ((n - n_f) * 77 + n_f * (255 - 77)) / (255 * n)) <= BAR
        assert np.array_equal(r["f_curve"][:78] > 0, np.ones(78, bool)) and not r["f_curve"][78:].any()          # b = 77: on up to k = 77
    # ... and a two-valued one is: 100 / 103 become 0 / 1
    two = np.where(m > 128, 103, 100).astype(np.uint8)
    assert from_pair(two, m, True)["mae"] == 0.0 and abs(from_pair(two, m, False)["mae"] - (n_f * 152 + (n - n_f) * 100) / (255 * n)) <= BAR


def test_split_point_rounds_half_up_and_may_sit_on_the_edge():
    m = np.zeros((1, 7), np.uint8)
    m[0, 2:4] = 255          # centroid 2.5: half up -> 3 (NumPy's round gives 2), cx = 4
    tables, head = R.tables_ref(np.full((1, 7), 9, np.uint8), m)
    assert head.tolist() == [2, 5, 0, 4, 1]
    assert int(np.round(2.5)) == 2
    # x < 4 on the left (two background, two foreground pixels), three background pixels on the right; cy = 1 = H: nothing below
    assert tables[0, :, 9].tolist() == [2, 2] and tables[1, :, 9].tolist() == [3, 0] and tables[2].sum() == 0 and tables[3].sum() == 0
    # cx = W, cy = H: the right and the lower quadrants are empty, without error
    m = np.zeros((5, 6), np.uint8)
    m[4, 5] = 255
    p = R.case("random", (5, 6))[0]
    tables, head = R.tables_ref(p, m)
    assert head[3:].tolist() == [6, 5] and tables[3].sum() == 0 and tables[1].sum() == 0 and tables[2].sum() == 0 and tables[0].sum() == 30
    got, want = S.per_image(tables[None], head[None], (5, 6)), R.image_ref(p, m)
    assert all(np.abs(got[k][0] - want[k]).max() <= BAR for k in want)
    assert R.tables_ref(p, np.zeros((5, 6), np.uint8))[1].tolist() == [0, 0, 0, 4, 3]          # no foreground: the middle


def test_dataset_reduction_is_the_maximum_of_the_mean_curve():
    pairs = [R.case("soft_block", (33, 65)), R.case("inverted", (33, 65)), R.case("random", (33, 65), seed=3)]
    pairs[1] = (np.where(pairs[1][1] > 128, 40, 10).astype(np.uint8), pairs[1][1])          # a faint but right prediction: raw F peaks low
    both = [R.tables_ref(p, m) for p, m in pairs]
    tables, head = np.stack([t for t, _ in both]), np.stack([h for _, h in both])
    for normalize in (True, False):
        res = S.metrics_from_tables(tables, head, (33, 65), normalize)
        per = S.per_image(tables, head, (33, 65), normalize)
        ref = R.dataset_ref(pairs, normalize)
        assert res["images"] == 3 and set(res) == set(S.KEYS) | {"images"}
        for k in S.KEYS:
            assert abs(res[k] - ref[k]) <= BAR, (k, res[k], ref[k])
        for curve, key_max, key_mean in (("f_curve", "max_f", "mean_f"), ("e_curve", "max_e", "mean_e")):
            assert res[key_max] == per[curve].mean(0).max() and abs(res[key_mean] - per[curve].mean()) <= BAR
    per = S.per_image(tables[:2], head[:2], (33, 65), False)          # two images whose F curves peak at different thresholds
    res = S.metrics_from_tables(tables[:2], head[:2], (33, 65), False)
    assert per["f_curve"][0].argmax() != per["f_curve"][1].argmax()
    assert per["f_curve"].max(1).mean() - res["max_f"] > 1e-3
    empty = S.metrics_from_tables(np.zeros((0, 4, 2, 256), np.int64), np.zeros((0, 5), np.int64), (1, 1))
    assert empty["images"] == 0 and all(np.isnan(empty[k]) for k in S.KEYS)


def test_per_image_refuses_a_table_that_is_not_its_images():
    tables, head = R.tables_ref(*R.case("random", (7, 13)))
    with pytest.raises(ValueError, match="expected 7x12 = 84"):
        S.per_image(tables[None], head[None], (7, 12))
    with pytest.raises(ValueError, match="head's nF"):
        S.per_image(tables[None], (head + np.array([1, 0, 0, 0, 0]))[None], (7, 13))
    sizes = np.array([[7, 13], [1, 1]])          # one size per image
    t1, h1 = R.tables_ref(*R.case("all_bg", (1, 1)))
    assert S.per_image(np.stack([tables, t1]), np.stack([head, h1]), sizes)["mae"].shape == (2,)


def test_golden_file_pins_the_definitions():
    assert os.path.getsize(R.GOLDEN) < 64 * 1024
    g = np.load(R.GOLDEN)
    report = json.load(open(R.REPORT))
    tags = sorted({k.split(".")[0] for k in g.files})
    assert len(tags) >= 8 and sorted(report) == tags
    for tag in tags:
        p, m = g[f"{tag}.pred"], g[f"{tag}.map"]
        family, shape = tag.rsplit("_", 1)[0], tuple(int(v) for v in tag.rsplit("_", 1)[1].split("x"))
        assert np.array_equal(p, R.case(family, shape)[0]) and np.array_equal(m, R.case(family, shape)[1])
        tables, head = R.tables_ref(p, m)
        assert np.array_equal(tables, g[f"{tag}.tables"]) and np.array_equal(head, g[f"{tag}.head"])
        for normalize, mode in ((True, "normalized"), (False, "raw")):
            values, f_curve, e_curve = g[f"{tag}.{mode}.values"], g[f"{tag}.{mode}.f_curve"], g[f"{tag}.{mode}.e_curve"]
            for got in (from_pair(p, m, normalize), R.image_ref(p, m, normalize)):
                assert np.abs(np.array([got[k] for k in ("mae", "s_measure", "adp_f", "adp_e")]) - values).max() <= BAR, (tag, mode)
                assert np.abs(got["f_curve"] - f_curve).max() <= BAR and np.abs(got["e_curve"] - e_curve).max() <= BAR, (tag, mode)
            assert report[tag][mode]["tables_vs_pixels"] <= BAR


def test_entry_point_is_declared_bound_and_refuses_before_launching():
    from adm_amd import hip
    header = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    decl = re.search(r"^int\s+adm_saliency_tables\s*\(([^;]*?)\)\s*;", header, flags=re.M | re.S)
    assert decl and len(decl.group(1).split(",")) == 9 == len(hip._SIGS["adm_saliency_tables"])          # (the stream included)
    assert "adm_saliency_tables" in hip.EXPORTS and "adm_saliency_tables" not in hip.NO_STREAM
    assert f"#define ADM_SALIENCY_BINS {S.BINS}" in header and "#define ADM_SALIENCY_MAX_PIXELS (1L << 24)" in header
    assert S.MAX_PIXELS == 1 << 24
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    fn = hip.lib().adm_saliency_tables
    a = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused before a launch
    ok = dict(pred=a, f32=0, map=a, tables=a, head=a, B=1, H=8, W=8)
    call = lambda **kw: fn(*{**ok, **kw}.values(), None)
    for bad in (dict(pred=None), dict(map=None), dict(tables=None), dict(head=None), dict(B=0), dict(B=65536), dict(H=0), dict(W=0),
                dict(H=-1), dict(H=4097, W=4096), dict(H=1, W=(1 << 24) + 1), dict(pred=ctypes.c_void_p(4098), f32=1)):
        assert call(**bad) == -22, bad


def test_sampling_field_is_off_on_every_other_row():
    from adm_amd.ddm import datasets
    from adm_amd.ddm.pair_data import DUTS_CLASSES
    assert datasets.Sampling._fields[-1] == "saliency" and datasets.SR_SAMPLING.saliency is False
    for key, row in datasets.DATASETS.items():
        if row.sampling is not None:
            assert row.sampling.saliency is (key == DUTS_CLASSES[0]), key
    assert datasets.DATASETS[DUTS_CLASSES[0]].sampling.gray and datasets.DATASETS[DUTS_CLASSES[0]].sampling.psnr          # (unchanged)


def test_samplers_refuse_the_key_on_another_data_set_and_no_yaml_sets_it():
    import sample_cond_dpm
    import sample_cond_ldm
    assert sample_cond_dpm.saliency_scorer is sample_cond_ldm.saliency_scorer
    duts = {"class_name": "ddm.data.DUTSDataset", "split": "test"}
    assert sample_cond_ldm.saliency_scorer(duts, {}) is None and sample_cond_ldm.saliency_scorer(duts, {"cal_saliency": False}) is None
    for flag, want in (({}, True), ({"saliency_normalize": False}, False)):
        score = sample_cond_ldm.saliency_scorer(duts, dict(flag, cal_saliency=True))
        assert isinstance(score, S.SaliencyScore) and score.normalize is want
    for other in ({"class_name": "ddm.data.InpaintDataset"}, {"class_name": "ddm.data.NYUDv2DepthDataset"}, {"class_name": "ddm.data.SketchDataset"},
                  {"class_name": "ddm.data.SRDatasetTest"}, {"class_name": "synthetic", "synthetic_of": "ddm.data.DUTSDataset"}, {}):
        with pytest.raises(ValueError, match="sampler.cal_saliency: True scores saliency maps"):
            sample_cond_ldm.saliency_scorer(other, {"cal_saliency": True})
        assert sample_cond_ldm.saliency_scorer(other, {}) is None
    # the pixel-space sampler asks before it refuses the data set in its own words
    src = inspect.getsource(sample_cond_dpm.main)
    assert 0 < src.index("saliency_scorer(cfg.data, s)") < src.index("check_dataset(cfg.data)")
    # opt-in: no committed YAML sets the key, so the samplers' save folders hold what they held
    for path in glob.glob(os.path.join(ROOT, "configs", "**", "*.yaml"), recursive=True):
        assert "cal_saliency" not in open(path).read(), path


def test_eval_saliency_refuses_a_missing_prediction_by_name(tmp_path):
    import eval_saliency
    img_dir, mask_dir = tmp_path / "DUTS-TE" / "DUTS-TE-Image", tmp_path / "DUTS-TE" / "DUTS-TE-Mask"
    img_dir.mkdir(parents=True), mask_dir.mkdir(parents=True), (tmp_path / "pred").mkdir()
    for name in ("a", "b"):
        (img_dir / f"{name}.jpg").write_bytes(b"")          # located, never opened: the refusal comes first
        (mask_dir / f"{name}.png").write_bytes(b"")
    (tmp_path / "pred" / "a.png").write_bytes(b"")
    with pytest.raises(FileNotFoundError, match=r"the prediction for .*b\.jpg is missing: .*pred.b\.png"):
        eval_saliency.main(["--pred", str(tmp_path / "pred"), "--data_root", str(tmp_path)])
    os.remove(mask_dir / "b.png")
    with pytest.raises(FileNotFoundError, match=r"the ground-truth map of .*b\.jpg is missing"):
        eval_saliency.main(["--pred", str(tmp_path / "pred"), "--data_root", str(tmp_path)])
