"""CPU-only: the host side of FID / Inception score (adm_amd/metrics, eval_fid.py and the opt-in keys of the unconditional drivers).
Golden values come from the reference's own metrics package (tools/make_golden_fid.py -> tests/golden/g26_fid.npz); nothing here
touches a GPU or a network."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g26_fid.npz")
REPORT = os.path.join(ROOT, "tests", "golden", "oracle_vs_reference_report_fid.json")
NEW = ("adm_conv_rect_relu_fwd", "adm_pool3x3_fwd", "adm_global_avgpool_fwd", "adm_tf1_resize_norm_u8", "adm_feat_stats_accum")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def test_new_symbols_are_declared_and_bound():
    from adm_amd import hip
    header = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    declared = set(re.findall(r"^(?:int|long)\s+(adm_\w+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in declared and name in hip._SIGS, name
    assert "inception.hip" in open(os.path.join(ROOT, "adm_amd", "csrc", "Makefile")).read()
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    for name in NEW:
        assert hasattr(hip.lib(), name), name


@pytest.mark.parametrize("shape,stride,pad", [((80, 64, 1, 1), 1, (0, 0)), ((24, 17, 1, 7), 1, (0, 3)), ((20, 9, 7, 1), 1, (3, 0)),
                                              ((16, 3, 3, 3), 2, (0, 0)), ((12, 7, 5, 5), 1, (2, 2))])
def test_bn_fold_matches_conv_then_batchnorm(shape, stride, pad):
    """fold_bn in float64 against plain float64 conv -> BatchNorm(eval, eps 1e-3) -> ReLU; and pack_rect's operand layout."""
    from adm_amd.metrics import inception as inc
    from oracle import fill
    co, ci, kh, kw = shape
    w = fill.hash_tensor(shape, "fold.w", 0.5, torch.float64)
    gamma = 1 + fill.hash_tensor((co,), "fold.g", 0.3, torch.float64)
    beta, mean = fill.hash_tensor((co,), "fold.b", 0.4, torch.float64), fill.hash_tensor((co,), "fold.m", 0.4, torch.float64)
    var = 1 + fill.hash_tensor((co,), "fold.v", 0.5, torch.float64)
    x = fill.hash_tensor((2, ci, 9, 11), "fold.x", 1.0, torch.float64)
    want = R.conv_bn_relu64(x, w, gamma, beta, mean, var, stride, pad)
    w64, b64 = inc.fold_bn(w, gamma, beta, mean, var)
    assert w64.dtype == torch.float64 and b64.dtype == torch.float64
    got = F.relu(F.conv2d(x, w64, b64, stride=stride, padding=pad))
    assert float((got > 0).double().mean()) > 0.2 and float((got == 0).double().mean()) > 0.2        # the ReLU cuts
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-13)
    wp, bp = inc.pack_rect(w64, b64, "cpu")
    cop, cip = inc.pad32(co), inc.pad32(ci)
    assert wp.shape == (cop, kh * kw * cip) and bp.shape == (cop,) and wp.dtype == torch.float32
    wp4 = wp.view(cop, kh, kw, cip)
    assert torch.equal(wp4[:co, :, :, :ci], w64.permute(0, 2, 3, 1).float())
    assert not wp4[co:].any() and not wp4[:, :, :, ci:].any() and not bp[co:].any()
    assert torch.equal(bp[:co], b64.float())


def test_state_dict_names_are_the_references(g):
    from adm_amd.metrics import inception as inc
    names = [str(n) for n in g["names"]]
    assert len(names) == 566
    m = inc.FeatureExtractorInceptionV3(["2048"])
    assert list(m.state_dict().keys()) == names == inc.state_dict_names()
    shapes = inc.state_dict_shapes()
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == shapes
    assert sum(int(np.prod(s)) for k, s in shapes.items() if not k.endswith("num_batches_tracked")) == 23885392
    sd = R.synthetic_state_dict({k: shapes[k] for k in ("Conv2d_1a_3x3.conv.weight", "fc.bias")})
    full = {k: torch.zeros(s, dtype=torch.long if k.endswith("tracked") else torch.float32) for k, s in shapes.items()}
    full.update(sd)
    m.load_state_dict(full, strict=True)
    assert torch.equal(m.Conv2d_1a_3x3.conv.weight, sd["Conv2d_1a_3x3.conv.weight"])
    missing = dict(full)
    del missing["Mixed_6c.branch7x7dbl_4.bn.running_var"]
    with pytest.raises(RuntimeError, match="Mixed_6c.branch7x7dbl_4.bn.running_var"):
        m.load_state_dict(missing, strict=True)
    extra = dict(full)
    extra["Mixed_7c.branch_pool.conv.bias"] = torch.zeros(192)
    with pytest.raises(RuntimeError, match="Mixed_7c.branch_pool.conv.bias"):
        m.load_state_dict(extra, strict=True)
    with pytest.raises(ValueError):
        inc.FeatureExtractorInceptionV3(["4096"])


def test_missing_weights_path_raises_and_opens_no_url(tmp_path, monkeypatch):
    import urllib.request
    import torch.hub
    from adm_amd.metrics import inception as inc

    def no_network(*a, **k):
        raise AssertionError("the extractor tried to fetch something")
    monkeypatch.setattr(urllib.request, "urlopen", no_network)
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", no_network)
    monkeypatch.setattr(torch.hub, "download_url_to_file", no_network)
    for path in (str(tmp_path / "absent.pth"), "", None):
        with pytest.raises(FileNotFoundError, match="does not exist"):
            inc.FeatureExtractorInceptionV3.from_file(path)


def test_fid_from_stats_matches_the_reference(g):
    from adm_amd.metrics import fid
    report = json.load(open(REPORT))["metrics"]
    for D, N1, N2 in R.METRIC_CASES:
        want, alt, d = (float(v) for v in g[f"metric.fid.{D}"])
        assert d <= 1e-6 and d == report[f"fid_{D}"]["d"], "ill-conditioned case: replace it in tools/make_golden_fid.py"
        st = [fid.Stats(*R.mean_cov64(R.metric_features(D, N, f"fid.metric.{D}.{k}")), N) for k, N in enumerate((N1, N2))]
        got = fid.fid_from_stats(st[0], st[1])
        print(f"D = {D}: got {got!r}, sqrtm {want!r}, eigen {alt!r}, d = {d:.2e}")
        assert abs(got - want) <= 100 * d * abs(want)
        assert fid.fid_from_stats({"mu": st[0].mu, "sigma": st[0].sigma}, st[1]) == got
    same = fid.fid_from_stats(st[0], st[0])
    assert abs(same) <= 1e-9 * float(np.trace(st[0].sigma))


def test_stats_save_load_roundtrip(tmp_path):
    from adm_amd.metrics import fid
    mu, sigma = R.mean_cov64(R.metric_features(64, 300, "fid.metric.64.0"))
    path = str(tmp_path / "stats.npz")
    fid.save_stats(path, fid.Stats(mu, sigma, 300))
    back = fid.FeatureStats.load(path)
    assert os.path.isfile(path) and back.n == 300 and back.mu.dtype == np.float64
    assert np.array_equal(back.mu, mu) and np.array_equal(back.sigma, sigma)


def test_inception_score_matches_the_reference(g):
    from adm_amd.metrics import fid
    got = fid.inception_score(R.isc_logits())
    want = g["metric.isc"]
    print(got, want)
    np.testing.assert_allclose([got["inception_score_mean"], got["inception_score_std"]], want, rtol=1e-12)
    assert set(got) == {"inception_score_mean", "inception_score_std"}
    unshuffled = fid.inception_score(R.isc_logits(), shuffle=False)
    assert unshuffled["inception_score_mean"] != got["inception_score_mean"]


def test_folder_listing_is_sorted_and_filtered(tmp_path):
    from PIL import Image
    from adm_amd.metrics import evaluate
    names = [" 000000010.png", " 000000002.png", "b.JPG", "a.jpeg", "notes.txt", "c.bmp"]
    for n in names:
        if n.endswith(".txt"):
            (tmp_path / n).write_text("x")
        else:
            Image.fromarray(np.full((4, 5, 3), 7, np.uint8)).save(str(tmp_path / n), format="PNG" if not n.endswith("bmp") else "BMP")
    (tmp_path / "sub.png").mkdir()
    got = [os.path.basename(p) for p in evaluate.list_images(str(tmp_path))]
    assert got == sorted(n for n in names if n.rsplit(".", 1)[1].lower() in ("png", "jpg", "jpeg"))
    assert got[0] == " 000000002.png"
    img = evaluate.load_u8(os.path.join(str(tmp_path), " 000000002.png"))
    assert img.dtype == torch.uint8 and tuple(img.shape) == (3, 4, 5) and int(img[0, 0, 0]) == 7
    with pytest.raises(FileNotFoundError):
        evaluate.list_images(str(tmp_path / "absent"))


def _weights_file(tmp_path):
    p = tmp_path / "w.pth"
    p.write_bytes(b"placeholder")         # the start-up checks only ask whether the file exists
    return str(p)


def test_drivers_refuse_more_than_one_process(tmp_path, monkeypatch):
    import eval_fid
    import sample_uncond
    import train_uncond_dpm
    from train_uncond_dpm import Cfg
    w = _weights_file(tmp_path)
    monkeypatch.setenv("WORLD_SIZE", "2")
    common = {"target_path": str(tmp_path), "inception_weights": w, "save_folder": str(tmp_path / "s"), "sample_num": 4,
              "batch_size": 2}
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        sample_uncond.check_cal_fid(Cfg({"sampler": dict(common, cal_fid=True)}))
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        train_uncond_dpm.check_test_in_train(Cfg({"sampler": dict(common, test_in_train=True)}))
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        eval_fid.main(["--input1", str(tmp_path), "--input2", str(tmp_path), "--weights", w])
    # without the keys nothing is refused: multi-process sampling and training stay as they were
    sample_uncond.check_cal_fid(Cfg({"sampler": dict(common)}))
    train_uncond_dpm.check_test_in_train(Cfg({"sampler": dict(common, test_in_train=False)}))
    train_uncond_dpm.check_test_in_train(Cfg({}))


def test_drivers_refuse_a_missing_weights_file(tmp_path, monkeypatch):
    import eval_fid
    import sample_uncond
    import train_uncond_dpm
    from train_uncond_dpm import Cfg
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    absent = str(tmp_path / "absent.pth")
    common = {"target_path": str(tmp_path), "save_folder": str(tmp_path / "s"), "sample_num": 4, "batch_size": 2}
    for weights in ({"inception_weights": absent}, {}):
        with pytest.raises(FileNotFoundError, match="weights file"):
            sample_uncond.check_cal_fid(Cfg({"sampler": dict(common, cal_fid=True, **weights)}))
        with pytest.raises(FileNotFoundError, match="weights file"):
            train_uncond_dpm.check_test_in_train(Cfg({"sampler": dict(common, test_in_train=True, **weights)}))
    with pytest.raises(FileNotFoundError, match="weights file"):
        eval_fid.main(["--input1", str(tmp_path), "--input2", str(tmp_path), "--weights", absent])
    w = _weights_file(tmp_path)
    with pytest.raises(FileNotFoundError, match="target_path"):
        sample_uncond.check_cal_fid(Cfg({"sampler": {"cal_fid": True, "inception_weights": w, "target_path": str(tmp_path / "no")}}))
    with pytest.raises(FileNotFoundError, match="target_path"):
        train_uncond_dpm.check_test_in_train(Cfg({"sampler": dict(common, test_in_train=True, inception_weights=w,
                                                                  target_path=str(tmp_path / "no"))}))


def test_no_shipped_config_turns_the_metrics_on():
    import glob
    import yaml
    for path in glob.glob(os.path.join(ROOT, "configs", "**", "*.yaml"), recursive=True):
        s = (yaml.load(open(path), Loader=yaml.SafeLoader) or {}).get("sampler") or {}
        assert not s.get("cal_fid") and not s.get("test_in_train"), path
