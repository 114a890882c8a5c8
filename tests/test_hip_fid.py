"""GPU: the kernels of csrc/inception.hip, the InceptionV3 extractor, the streaming statistics and the FID / Inception-score drivers.

Convolutions and pools are checked against float64 arithmetic computed here on the CPU; the resize, the whole extractor and the
end-to-end metrics against the reference's own results in tests/golden/g26_fid.npz (tools/make_golden_fid.py).  The weights are the
synthetic state dict of tests/inception_ref.py, rebuilt from its hash, once per module."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import inception_ref as R
import parity
from oracle import fill

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g26_fid.npz")
GOLDEN_RESIZE = os.path.join(ROOT, "tests", "golden", "g26_fid_resize.npz")
REPORT = os.path.join(ROOT, "tests", "golden", "oracle_vs_reference_report_fid.json")
KEYS = {"frechet_inception_distance", "inception_score_mean", "inception_score_std"}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def inc():
    from adm_amd.metrics import inception
    return inception


@pytest.fixture(scope="module")
def state_dict(inc):
    return R.synthetic_state_dict(inc.state_dict_shapes())


@pytest.fixture(scope="module")
def net(gpu, inc, state_dict):
    m = inc.FeatureExtractorInceptionV3(list(R.FEATURES))
    m.load_state_dict(state_dict, strict=True)
    return m.to(gpu)


@pytest.fixture(scope="module")
def weights_file(tmp_path_factory, state_dict):
    path = str(tmp_path_factory.mktemp("inception") / "synthetic_inception.pth")
    torch.save(state_dict, path)
    return path


def nhwc_pad(x, dev):
    """NCHW -> NHWC f32 with the channels zero-padded to a multiple of 32"""
    B, C, H, W = x.shape
    y = torch.zeros(B, H, W, (C + 31) // 32 * 32, dtype=torch.float32)
    y[..., :C] = x.permute(0, 2, 3, 1)
    return y.to(dev)


# ------------------------------------------------------------------------------------------------------------ convolution
# (id, (kh, kw), stride, (pad_h, pad_w), cin, cout, (H, W), B)
CONV_CASES = [
    ("3x3s2_3to32", (3, 3), 2, (0, 0), 3, 32, (19, 23), 2),
    ("3x3_32to32", (3, 3), 1, (0, 0), 32, 32, (9, 11), 2),
    ("3x3p1_32to64", (3, 3), 1, (1, 1), 32, 64, (9, 11), 2),
    ("1x1_64to80", (1, 1), 1, (0, 0), 64, 80, (9, 11), 2),
    ("1x1_80to192", (1, 1), 1, (0, 0), 80, 192, (9, 11), 2),
    ("5x5p2_48to64", (5, 5), 1, (2, 2), 48, 64, (9, 11), 2),
    ("1x7_160_17x17", (1, 7), 1, (0, 3), 160, 160, (17, 17), 2),
    ("1x7_160_5x9", (1, 7), 1, (0, 3), 160, 160, (5, 9), 2),
    ("7x1_160to192_17x17", (7, 1), 1, (3, 0), 160, 192, (17, 17), 2),
    ("7x1_160to192_5x9", (7, 1), 1, (3, 0), 160, 192, (5, 9), 2),
    ("3x3s2_288to384", (3, 3), 2, (0, 0), 288, 384, (17, 17), 2),
    ("3x3p1_448to384_longestK", (3, 3), 1, (1, 1), 448, 384, (8, 8), 1),
    ("1x7_128_M867", (1, 7), 1, (0, 3), 128, 128, (17, 17), 3),
]


def conv_case(inc, tag, k, stride, pad, ci, co, hw, B):
    """inputs of both signs, a non-zero folded bias; -> (x NCHW f32, packed operands, float64 reference NCHW, max sum|ab|)"""
    x = fill.hash_tensor((B, ci, *hw), tag + ".x", 1.0)
    w = fill.hash_tensor((co, ci, *k), tag + ".w", (6.0 / (ci * k[0] * k[1])) ** 0.5)
    gamma, beta = 1 + fill.hash_tensor((co,), tag + ".g", 0.1), fill.hash_tensor((co,), tag + ".b", 0.3)
    mean, var = fill.hash_tensor((co,), tag + ".m", 0.3), 1 + fill.hash_tensor((co,), tag + ".v", 0.5)
    want = R.conv_bn_relu64(x, w, gamma, beta, mean, var, stride, pad)
    w64, b64 = inc.fold_bn(w, gamma, beta, mean, var)
    scale = float((F.conv2d(x.double().abs(), w64.abs(), None, stride=stride, padding=pad) + b64.abs()[None, :, None, None]).max())
    cut = float((want == 0).double().mean())
    assert 0.1 < cut < 0.9, f"{tag}: the ReLU cuts {cut:.0%} of the outputs"
    return x, w64, b64, want, scale


def check_conv(got_nhwc, want, scale, co, tag):
    got = got_nhwc[..., :co].permute(0, 3, 1, 2).cpu()
    err = float((got.double() - want).abs().max()) / scale
    print(f"{tag}: error vs float64 = {err:.2e} of max sum|ab| (bar 4e-7)")
    parity.close(got, want)
    assert err <= 4e-7
    assert not got_nhwc[..., co:].any(), f"{tag}: padded output lanes must be written as zero"


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_rect_against_float64(gpu, inc, case):
    tag, k, stride, pad, ci, co, hw, B = case
    x, w64, b64, want, scale = conv_case(inc, tag, k, stride, pad, ci, co, hw, B)
    wp, bp = inc.pack_rect(w64, b64, gpu)
    cop = inc.pad32(co)
    out = torch.full((B, want.shape[2], want.shape[3], cop), float("nan"), device=gpu)       # every lane must be written
    got = inc.conv_rect(nhwc_pad(x, gpu), wp, bp, k, stride, pad, out=out)
    assert tuple(got.shape) == (B, want.shape[2], want.shape[3], cop)
    check_conv(got, want, scale, co, tag)


@pytest.mark.parametrize("tile", [0, 1, 2, 3])
def test_conv_rect_every_tile_on_a_ragged_shape(gpu, inc, tile):
    """each launch plan (128x128, 128x96, 64x64, 128x32) on M = 867 and 160 output channels: ragged against every tile"""
    tag, k, stride, pad, ci, co, hw, B = ("tiles", (7, 1), 1, (3, 0), 96, 160, (17, 17), 3)
    x, w64, b64, want, scale = conv_case(inc, tag, k, stride, pad, ci, co, hw, B)
    wp, bp = inc.pack_rect(w64, b64, gpu)
    got = inc.conv_rect(nhwc_pad(x, gpu), wp, bp, k, stride, pad, tile=tile)
    check_conv(got, want, scale, co, f"tile {tile}")


def test_conv_rect_writes_slices_of_a_wider_buffer(gpu, inc):
    """1x3 and 3x1, 384 -> 384 on 8x8, at offsets 0 and 384 of a 768-wide buffer: the sentinel in every other lane stays"""
    B, hw, ci, co = 2, (8, 8), 384, 384
    sentinel = -12345.0
    out = torch.full((B, 8, 8, 768), sentinel, device=gpu)
    parts = []
    for tag, k, pad, off in (("slice.1x3", (1, 3), (0, 1), 0), ("slice.3x1", (3, 1), (1, 0), 384)):
        xc, w64, b64, want, scale = conv_case(inc, tag, k, 1, pad, ci, co, hw, B)
        x = nhwc_pad(xc, gpu)
        wp, bp = inc.pack_rect(w64, b64, gpu)
        before = out.clone()
        inc.conv_rect(x, wp, bp, k, 1, pad, out=out, yoff=off)
        other = slice(384, 768) if off == 0 else slice(0, 384)
        assert torch.equal(out[..., other], before[..., other]), f"{tag}: lanes outside the slice changed"
        check_conv(out[..., off:off + co], want, scale, co, tag)
        parts.append(out[..., off:off + co].clone())
    assert torch.equal(out[..., :384], parts[0]) and not (out == sentinel).any()
    # reading a slice: the second half of the 768-wide buffer as the input of a 1x1 conv
    xs = out[..., 384:]
    w = fill.hash_tensor((64, 384, 1, 1), "slice.read.w", (6.0 / 384) ** 0.5)
    wp, bp = inc.pack_rect(w.double(), fill.hash_tensor((64,), "slice.read.b", 0.3).double(), gpu)
    wide = out.clone()
    got = torch.empty(B, 8, 8, 64, device=gpu)
    from adm_amd import hip
    hip.call("adm_conv_rect_relu_fwd", wide.data_ptr() + 384 * 4, hip.ptr(wp), hip.ptr(bp), hip.ptr(got), B, 8, 8, 384, 768, 64, 64,
             0, 1, 1, 1, 0, 0, 1, -1)
    want = inc.conv_rect(xs.contiguous(), wp, bp, (1, 1))
    assert torch.equal(got, want)


def test_conv_rect_rejects_what_it_cannot_run(gpu, inc):
    from adm_amd import hip
    x = torch.zeros(1, 8, 8, 32, device=gpu)
    wp = torch.zeros(32, 9 * 32, device=gpu)
    y = torch.zeros(1, 8, 8, 64, device=gpu)

    def rc(**kw):
        a = dict(B=1, H=8, W=8, cin=32, ldx=32, N=32, ldy=64, yoff=0, kh=3, kw=3, stride=1, ph=1, pw=1)
        a.update(kw)
        return hip.lib().adm_conv_rect_relu_fwd(hip.ptr(x), hip.ptr(wp), None, hip.ptr(y), a["B"], a["H"], a["W"], a["cin"], a["ldx"],
                                                a["N"], a["ldy"], a["yoff"], a["kh"], a["kw"], a["stride"], a["ph"], a["pw"], 1, -1,
                                                hip.stream())
    assert rc() == 0
    for bad in (dict(kh=2), dict(kw=9), dict(stride=3), dict(ph=2), dict(cin=16), dict(N=48), dict(yoff=16), dict(yoff=64),
                dict(N=96), dict(ldx=16)):
        assert rc(**bad) == -22, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ pooling
def _pool_ref(x, mode):
    xd = x.double()
    if mode == 0:
        return F.max_pool2d(xd, 3, 2)
    if mode == 1:
        return F.max_pool2d(xd, 3, 1, 1)
    return F.avg_pool2d(xd, 3, 1, 1, count_include_pad=False)


@pytest.mark.parametrize("C", [32, 288])
@pytest.mark.parametrize("mode,hw", [(0, (9, 11)), (0, (8, 8)), (2, (1, 1)), (2, (2, 2)), (2, (5, 7)), (1, (5, 7))])
def test_pool3x3(gpu, inc, mode, hw, C):
    x = fill.hash_tensor((2, C, *hw), f"pool.{mode}.{hw}", 1.0)
    if mode == 1:
        x = x - 2.0            # an all-negative map: zero padding would win every border maximum
    want = _pool_ref(x, mode)
    xg = nhwc_pad(x, gpu)
    got = inc.pool3x3(xg, mode).permute(0, 3, 1, 2).cpu()
    if mode == 2:
        if hw == (5, 7):       # the divisors 4, 6 and 9 all occur (1 on 1x1, 4 on 2x2)
            cnt = F.avg_pool2d(torch.ones(1, 1, *hw), 3, 1, 1, count_include_pad=True) * 9
            assert sorted(set(cnt.round().int().flatten().tolist())) == [4, 6, 9]
        parity.close(got, want)
        assert float((got.double() - want).abs().max()) <= 9 * 2.0 ** -24 * float(x.abs().max())      # eight f32 adds of partial sums <= 9 max|x|, a divide by 9
    else:
        assert torch.equal(got.double(), want)
        assert mode != 1 or float(got.max()) < 0
    # the same into a slice of a wider buffer
    sentinel = 777.0
    wide = torch.full((2, want.shape[2], want.shape[3], C + 64), sentinel, device=gpu)
    inc.pool3x3(xg, mode, out=wide, yoff=32)
    assert torch.equal(wide[..., 32:32 + C].permute(0, 3, 1, 2).cpu(), got)
    assert bool((wide[..., :32] == sentinel).all()) and bool((wide[..., 32 + C:] == sentinel).all())


@pytest.mark.parametrize("C", [32, 288])
@pytest.mark.parametrize("hw", [(8, 8), (7, 5)])
def test_global_avgpool(gpu, inc, hw, C):
    x = fill.hash_tensor((2, C, *hw), f"gap.{hw}", 1.0) + 0.25
    want = x.double().mean((2, 3))
    xg = nhwc_pad(x, gpu)
    got = inc.global_avgpool(xg).cpu()
    parity.close(got, want)
    assert float((got.double() - want).abs().max()) <= 2.0 ** -24 * float(want.abs().max()) * 1.01      # float64 sum, one rounding
    assert torch.equal(inc.global_avgpool(xg).cpu(), got)
    # the first 32 channels of a wider tensor
    assert torch.equal(inc.global_avgpool(xg, C=32).cpu(), got[:, :32])


# ------------------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("hw", R.RESIZE_SHAPES, ids=[f"{h}x{w}" for h, w in R.RESIZE_SHAPES])
def test_tf1_resize_is_bit_equal_to_the_reference(gpu, inc, g, hw):
    H, W = hw
    img = R.images_u8((1, 3, H, W), f"fid.resize.{H}x{W}")
    out = inc.tf1_resize_norm(img.to(gpu))
    assert tuple(out.shape) == (1, 299, 299, 32) and not out[..., 3:].any()
    got = out[..., :3].permute(0, 3, 1, 2).cpu().numpy()
    if hw == R.RESIZE_SHAPES[0]:
        want = np.concatenate([np.load(GOLDEN_RESIZE)[f"resize.{H}x{W}.c01"], g[f"resize.{H}x{W}.c2"]], axis=1)
    else:
        idx = R.sub_idx(299)
        got, want = got[:, :, idx][:, :, :, idx], g[f"resize.{H}x{W}"]
    assert got.shape == want.shape and want.dtype == np.float32
    diff = got.view(np.int32) != want.view(np.int32)
    print(f"{H}x{W}: {int(diff.sum())} of {diff.size} values differ in their bits")
    assert not diff.any()


# ------------------------------------------------------------------------------------------------------------ whole extractor
@pytest.mark.parametrize("case", R.EXTRACT_CASES, ids=[c[0] for c in R.EXTRACT_CASES])
def test_extractor_against_the_reference_in_float64(gpu, net, g, case):
    """Bars: parity.close, and error over max|ref| at most max(4 * e32, 2e-6), e32 being the reference's own float32 error against
    its float64 run (the rule of smoke())."""
    tag, B, H, W = case
    report = json.load(open(REPORT))["extractor"][tag]
    img = R.images_u8((B, 3, H, W), f"fid.extract.{tag}").to(gpu)
    taps = {}
    net.features_list = list(R.FEATURES)
    out = net(img, taps=taps)
    for name, t in taps.items():          # printed before any assertion: locates a failure
        want = g[f"extract.{tag}.tap.{name}"]
        print(f"  {name}: spatial-mean error {float(np.abs(t.cpu().numpy()[:, :want.shape[1]] - want).max() / np.abs(want).max()):.2e}")
    again = net(img)
    errs = {}
    for name, got, got2 in zip(R.FEATURES, out, again):
        want = g[f"extract.{tag}.{name}"]
        assert tuple(got.shape) == want.shape and got.dtype == torch.float32
        e32 = report[name]["e32"]
        errs[name] = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max())
        print(f"{tag} {name}: error {errs[name]:.2e} of max|ref| (reference float32: {e32:.2e}; bar {max(4 * e32, 2e-6):.2e})")
        assert torch.equal(got, got2), f"{name}: two runs differ"
    for name, got in zip(R.FEATURES, out):
        parity.close(got, g[f"extract.{tag}.{name}"])
        assert errs[name] <= max(4 * report[name]["e32"], 2e-6), name
    assert report["nonzero_share_2048"] >= 0.5


def test_extractor_returns_after_the_last_requested_feature(gpu, net, g, monkeypatch):
    from adm_amd import hip
    calls = []
    real = hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    tag, B, H, W = R.EXTRACT_CASES[0]
    img = R.images_u8((B, 3, H, W), f"fid.extract.{tag}").to(gpu)
    try:
        net.features_list = ["64"]
        out = net(img)
        assert len(out) == 1 and tuple(out[0].shape) == (B, 64)
        assert calls.count("adm_conv_rect_relu_fwd") == 3 and calls.count("adm_pool3x3_fwd") == 1, calls
        net.features_list = ["logits", "64"]            # the order of the list is the order of the tuple
        full = net(img)
        assert tuple(full[0].shape) == (B, 1008) and torch.equal(full[1], out[0])
        assert calls.count("adm_conv_rect_relu_fwd") == 3 + 94 + 1
    finally:
        net.features_list = list(R.FEATURES)
    with pytest.raises(ValueError):
        net(img.float())


# ------------------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("offset,tol", [(0.0, 1e-12), (1e5, 1e-11)])
@pytest.mark.parametrize("D", [64, 2048])
def test_feature_stats_against_numpy(gpu, D, offset, tol):
    """N = 37 in batches of 16, 16 and 5 against np.mean / np.cov of the float64-cast values; with 1e5 added to every feature the
    unshifted one-pass form would lose about six digits."""
    from adm_amd.metrics import fid
    x = (fill.hash_tensor((37, D), f"stats.{D}", 1.0) * (1 + fill.hash_tensor((1, D), f"stats.{D}.s", 0.9).abs()) + offset).float()
    mu, sigma = R.mean_cov64(x.numpy())
    runs = []
    for _ in range(2):
        st = fid.FeatureStats(D, gpu)
        for lo, hi in ((0, 16), (16, 32), (32, 37)):
            st.update(x[lo:hi].to(gpu))
        runs.append(st.finalize())
    got = runs[0]
    assert got.n == 37 and got.mu.dtype == np.float64 and got.sigma.dtype == np.float64
    smax = float(np.abs(sigma).max())
    e_mu, e_sg = float(np.abs(got.mu - mu).max()), float(np.abs(got.sigma - sigma).max())
    print(f"D = {D}, offset {offset:g}: mu error {e_mu:.2e}, sigma error {e_sg:.2e} = {e_sg / smax:.2e} of max|sigma|")
    assert e_sg <= tol * smax and e_mu <= tol * max(1.0, float(np.abs(mu).max()))
    assert np.array_equal(got.mu, runs[1].mu) and np.array_equal(got.sigma, runs[1].sigma), "two runs differ"
    assert np.array_equal(got.sigma, got.sigma.T)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_fid_end_to_end_against_the_reference(gpu, net, g):
    """|FID - want64| <= 4 |want32 - want64| + 1e-6 |want64|: four times the reference's own float32 error, with a floor far below the
    two decimals FID is quoted to."""
    from adm_amd.metrics import fid
    want64, want32 = (float(v) for v in g["e2e.fid"])
    stats = []
    try:
        net.features_list = ["64"]
        for s in R.e2e_sets():
            st = fid.FeatureStats(64, gpu)
            for i in range(0, s.shape[0], 100):
                st.update(net(s[i:i + 100].to(gpu))[0])
            stats.append(st.finalize())
    finally:
        net.features_list = list(R.FEATURES)
    got = fid.fid_from_stats(stats[0], stats[1])
    print(f"FID {got!r}; reference float64 {want64!r}, float32 {want32!r}; bar {4 * abs(want32 - want64) + 1e-6 * abs(want64):.2e}, "
          f"off by {abs(got - want64):.2e}")
    assert abs(got - want64) <= 4 * abs(want32 - want64) + 1e-6 * abs(want64)


def test_inception_score_end_to_end_against_the_reference(gpu, net, g):
    """Mean held as the FID is.  The std of the split scores is in the scores' units, so its floor is 1e-6 of the MEAN: an error
    of the scores moves their std by at most as much."""
    from adm_amd.metrics import fid
    (m64, s64), (m32, s32) = g["e2e.isc"].tolist()
    sub = R.e2e_sets()[0][:R.E2E_ISC_N]
    try:
        net.features_list = ["logits"]
        logits = net(sub.to(gpu))[0]
    finally:
        net.features_list = list(R.FEATURES)
    got = fid.inception_score(logits, splits=R.E2E_ISC_SPLITS)
    print(f"Inception score {got}; reference float64 ({m64!r}, {s64!r}), float32 ({m32!r}, {s32!r})")
    assert abs(got["inception_score_mean"] - m64) <= 4 * abs(m32 - m64) + 1e-6 * abs(m64)
    assert abs(got["inception_score_std"] - s64) <= 4 * abs(s32 - s64) + 1e-6 * abs(m64)


def _write_pngs(folder, imgs):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for i, a in enumerate(imgs.permute(0, 2, 3, 1).numpy()):
        Image.fromarray(a).save(os.path.join(folder, f"{i: 010d}.png"))


def test_cli_eval_fid_on_two_folders(gpu, net, weights_file, tmp_path):
    from adm_amd.metrics import fid
    a, b = (s[:12] for s in R.e2e_sets())
    _write_pngs(str(tmp_path / "a"), a)
    _write_pngs(str(tmp_path / "b"), b)
    out, stats = str(tmp_path / "out" / "result.json"), str(tmp_path / "a_stats.npz")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval_fid.py"), "--input1", str(tmp_path / "a"), "--input2", str(tmp_path / "b"),
                        "--weights", weights_file, "--isc", "--batch-size", "8", "--out_path", out, "--save-stats", stats],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.load(open(out))
    assert set(res) == KEYS and json.loads(r.stdout.strip().splitlines()[-1]) == res
    assert all(np.isfinite(v) for v in res.values()) and res["frechet_inception_distance"] > 0 and res["inception_score_mean"] >= 1
    # the same numbers from this process: PNG is lossless, so the folders hold the bytes of a and b
    st = []
    try:
        for s, feats in ((a, ["2048", "logits"]), (b, ["2048"])):
            net.features_list = feats
            acc, rows = fid.FeatureStats(2048, gpu), []
            for i in range(0, 12, 8):
                o = net(s[i:i + 8].to(gpu))
                acc.update(o[0])
                rows += [o[1].cpu()] if len(o) > 1 else []
            st.append((acc.finalize(), rows))
    finally:
        net.features_list = list(R.FEATURES)
    assert res["frechet_inception_distance"] == fid.fid_from_stats(st[0][0], st[1][0])
    assert res["inception_score_mean"] == fid.inception_score(torch.cat(st[0][1]))["inception_score_mean"]
    saved = fid.load_stats(stats)
    assert saved.n == 12 and np.array_equal(saved.mu, st[0][0].mu) and np.array_equal(saved.sigma, st[0][0].sigma)


def _small_cifar_cfg(tmp_path, weights_file):
    cfg = yaml.load(open(os.path.join(ROOT, "configs", "cifar10", "ddm_uncond_const_uncond_unet.yaml")), Loader=yaml.SafeLoader)
    cfg["model"]["unet"].update(model_channels=64, num_blocks=1)
    target = str(tmp_path / "target")
    _write_pngs(target, R.e2e_sets()[1][:12])
    res = str(tmp_path / "run")
    cfg["sampler"].update(batch_size=12, sample_num=12, save_folder=os.path.join(res, "png"), target_path=target,
                          inception_weights=weights_file)
    return cfg, res, target


def test_cli_sample_uncond_with_cal_fid(gpu, weights_file, tmp_path):
    cfg, res, target = _small_cifar_cfg(tmp_path, weights_file)
    cfg["sampler"].update(cal_fid=True, sample_num=24)
    path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sample_uncond.py"), "--cfg", path, "--random-init", "--max-batches", "1"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(os.path.join(res, "png"))) == sorted([f"{i: 010d}.png" for i in range(12)] + ["result.json"])
    out = json.load(open(os.path.join(res, "png", "result.json")))
    assert set(out) == KEYS and all(np.isfinite(v) for v in out.values()) and out["frechet_inception_distance"] > 0
    assert os.path.isfile(target + ".npz"), "the target statistics are cached next to target_path"


def test_cli_train_uncond_with_test_in_train(gpu, weights_file, tmp_path):
    cfg, res, target = _small_cifar_cfg(tmp_path, weights_file)
    cfg["data"] = {"class_name": "synthetic", "batch_size": 8, "image_size": [32, 32]}
    cfg["trainer"].update(results_folder=res, train_num_steps=2, save_and_sample_every=2, log_freq=1, test_before=False,
                          ema_update_after_step=1, ema_update_every=1)
    cfg["sampler"].update(test_in_train=True)
    path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_uncond_dpm.py"), "--cfg", path, "--max-steps", "2"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(os.path.join(res, "png"))) == [f"{i: 010d}.png" for i in range(12)]
    out = json.load(open(os.path.join(res, "result_1.json")))
    assert set(out) == KEYS and all(np.isfinite(v) for v in out.values())
    assert os.path.isfile(target + ".npz") and os.path.exists(os.path.join(res, "model-1.pt"))
