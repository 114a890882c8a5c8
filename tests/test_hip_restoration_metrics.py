"""GPU: the restoration score (adm_restoration_sums, adm_amd/metrics/restoration.py, eval_restoration.py, sampler.cal_restoration).

Bars.  The SSE words are integers: they must EQUAL the restatement's Python integers (tests/restoration_ref.py).  Per-plane SSIM is
held to 1e-10 absolute of the restatement's direct 2-D window.  Derivation: a filtered second moment is a sum of 121 products of
magnitude up to 65025 with weights summing to 1, rounded about two dozen times on the separable route (11 + 11 adds, as many
multiplies): 24 x 2^-53 x 65025 = 1.7e-10 at the very worst on a variance term w*x^2 - mu^2, which enters the value divided by a
denominator of at least C2 = 58.5 and multiplied by a factor of at most 2: under 1e-11, a decade inside the bar, and roundings do not
all align.  The same quantity on the CPU -- the separable float64 order against the direct window -- measures at most 2.5e-12 (flat
255 / 254, tests/golden/g32_restoration_report.json).  A float32 filter is 6.7e-5 off (tests/test_restoration_host.py).  The mean over
the positions adds n 2^-53 relative at worst, 4e-13 for the largest shape here.  The worst deviation seen is printed by every case and
recorded by tools/restoration_metrics_cost.py.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import restoration_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, SHAPES = R.TILE, R.GPU_SHAPES
DTYPES = [(torch.uint8, torch.uint8), (torch.float32, torch.uint8), (torch.uint8, torch.float32), (torch.float32, torch.float32)]
SENTINEL, GUARD = -7, 16


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip
    hip.lib()
    assert hip.lib().adm_restoration_blocks(T + 10, T + 10) == 1 and hip.lib().adm_restoration_blocks(T + 11, T + 10) == 2
    return torch.device("cuda:0")


def as_dtype(x, dtype, gpu):
    t = torch.from_numpy(np.array(x)).to(gpu)
    return t if dtype == torch.uint8 else (t.float() / 255).contiguous()          # (k / 255 * 255 rounds back to k)


def launch(gpu, pred, target, s):
    """The raw call on sentinel-filled outputs between guard bands -> (sse [B,P,2], ssim sums [B,P]); the payload must be overwritten
    whole, the guards left, the ticket zero again."""
    from adm_amd import hip
    B, C, H, W = pred.shape
    P = 4 if C == 3 else 1
    blocks = int(hip.lib().adm_restoration_blocks(H - 2 * s, W - 2 * s))
    sse = torch.full((GUARD + B * P * 2 + GUARD,), SENTINEL, device=gpu, dtype=torch.int64)
    ssim = torch.full((GUARD + B * P + GUARD,), float(SENTINEL), device=gpu, dtype=torch.float64)
    partial = torch.full((B * blocks * P * 2,), SENTINEL, device=gpu, dtype=torch.int64)
    ticket = torch.zeros(GUARD + B + GUARD, device=gpu, dtype=torch.int32)
    ticket[:GUARD], ticket[GUARD + B:] = SENTINEL, SENTINEL
    hip.call("adm_restoration_sums", hip.ptr(pred), int(pred.dtype == torch.float32), hip.ptr(target), int(target.dtype == torch.float32),
             hip.ptr(sse[GUARD:]), hip.ptr(ssim[GUARD:]), hip.ptr(partial), hip.ptr(ticket[GUARD:]), B, C, H, W, s)
    sse, ssim, ticket = sse.cpu().numpy(), ssim.cpu().numpy(), ticket.cpu().numpy()
    for buf, n in ((sse, B * P * 2), (ssim, B * P), (ticket, B)):
        assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all(), "a guard band was written"
    assert (ticket[GUARD:GUARD + B] == 0).all(), "the ticket is not zero on return"
    sse, ssim = sse[GUARD:GUARD + B * P * 2].reshape(B, P, 2), ssim[GUARD:GUARD + B * P].reshape(B, P)
    assert (sse[..., 0] >= 0).all() and (sse[..., 0] < (1 << 32)).all() and (sse[..., 1] >= 0).all() and np.isfinite(ssim).all()
    return sse, ssim


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("hw,B", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"B{v}")
def test_sums_equal_the_restatement(gpu, hw, B, family):
    """Every channel count, shave and input type of one shape and data family: SSE words exactly, per-plane SSIM within the bar, through
    the wrapper and through the raw ABI, twice with identical bits."""
    from adm_amd.metrics.restoration import per_image, restoration_sums
    worst = 0.0
    for C in (1, 3):
        for s in (0, 4):
            p, g, want = R.batch_ref(family, hw, B, C, s)
            want_words = np.stack([R.words(r["sse"]) for r in want])
            want_ssim = np.stack([r["ssim_planes"] for r in want])
            count = (hw[0] - 10) * (hw[1] - 10)
            first = None
            for pt, gt in DTYPES:
                pd, gd = as_dtype(p, pt, gpu), as_dtype(g, gt, gpu)
                sse, ssim = restoration_sums(pd, gd, s)
                assert sse.dtype == torch.int64 and tuple(sse.shape) == (B, want_words.shape[1], 2) and ssim.dtype == torch.float64
                got_words, got_sums = sse.cpu().numpy(), ssim.cpu().numpy()
                assert np.array_equal(got_words, want_words), (C, s, pt, gt, got_words.tolist(), want_words.tolist())
                gap = float(np.abs(got_sums / count - want_ssim).max())
                worst = max(worst, gap)
                assert gap <= R.BAR, (C, s, pt, gt, gap)
                if first is None:
                    first = got_sums
                assert np.array_equal(got_sums.view(np.int64), first.view(np.int64))          # the input's type changes no bit
                raw_words, raw_sums = launch(gpu, pd, gd, s)
                assert np.array_equal(raw_words, got_words) and np.array_equal(raw_sums.view(np.int64), got_sums.view(np.int64))
            m = per_image(got_words, got_sums, hw)
            for i, r in enumerate(want):
                assert list(m["sse_planes"][i]) == r["sse"]
                for k in (R.KEYS if C == 3 else R.KEYS[:2]):
                    assert m[k][i] == r[k] or abs(m[k][i] - r[k]) <= R.BAR, (k, m[k][i], r[k])
            if family == "equal":          # exactly 1 and inf, not nearly
                assert (got_sums == float(count)).all() and (got_words == 0).all()
                assert (m["ssim"] == 1.0).all() and (m["psnr"] == math.inf).all()
                assert C == 1 or ((m["ssim_y"] == 1.0).all() and (m["psnr_y"] == math.inf).all())
    print(f"worst per-plane SSIM deviation from the restatement: {worst:.3g} (bar {R.BAR:g})")


def test_fringe_pixels_have_exactly_one_owner(gpu):
    """One differing pixel on 2 x 3 ragged tiles, placed on either side of every tile seam, in the last 10 rows, the last 10 columns and
    the corner: wherever it is, the SSE is that pixel's square -- counted once, by one tile.  (The `fringe` family of
    test_sums_equal_the_restatement differs in the whole fringe and nowhere else.)"""
    from adm_amd.metrics.restoration import restoration_sums
    H, W = T + 23, 2 * T + 23
    g = np.full((1, 1, H, W), 100, np.uint8)
    for y, x in ((0, 0), (T - 1, T - 1), (T, T), (T + 12, T), (T + 13, 2 * T + 12), (T + 13, 2 * T + 13), (H - 1, W - 1), (H - 11, W - 1),
                 (H - 1, W - 11), (H - 10, 0), (0, W - 10), (T + 12, 2 * T + 22), (T + 22, 2 * T + 12), (T - 1, 2 * T - 1), (T, 2 * T)):
        p = g.copy()
        p[0, 0, y, x] = 107
        sse, _ = restoration_sums(torch.from_numpy(p).to(gpu), torch.from_numpy(g).to(gpu))
        assert sse[0, 0].tolist() == [49, 0], (y, x, sse[0, 0].tolist())


def test_float32_inputs_are_quantised_as_the_png_writer_does(gpu):
    """The bytes scored are (v.clamp(0, 1) * 255).round() of torch: values below 0 and above 1, float32 values whose product with 255 is an
    exact half (ties to even: both an even and an odd neighbour below), and NaN as byte 0 -- on the prediction and on the target, from a
    buffer one float off its 16-byte boundary as well."""
    import saliency_ref as SR
    from adm_amd.metrics.restoration import restoration_sums
    halves = SR.half_floats()
    k = (halves.astype(np.float32) * np.float32(255.0)).astype(np.int64)
    assert len(halves) >= 16 and (k % 2 == 0).any() and (k % 2 == 1).any()
    B, C, H, W = 2, 3, 19, 23
    rng = np.random.default_rng(11)
    vals = rng.uniform(-0.5, 1.5, B * C * H * W).astype(np.float32)
    special = np.concatenate([halves, np.float32([-0.0, 0.0, 1.0, -3.0, 7.5, 1e-30, -1e30, 1e30, np.inf, -np.inf, 0.5, 1.0 / 255])])
    vals[:len(special)] = special
    vals = vals[rng.permutation(vals.size)]
    other = rng.integers(0, 256, (B, C, H, W)).astype(np.uint8)
    for offset in (0, 1):
        buf = torch.zeros(B * C * H * W + 4, device=gpu, dtype=torch.float32)
        fd = buf[offset:offset + B * C * H * W].view(B, C, H, W)
        fd.copy_(torch.from_numpy(vals).view(B, C, H, W))
        assert fd.data_ptr() % 16 == 4 * offset
        want_bytes = (fd.clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
        assert np.array_equal(want_bytes, R.quantise(vals).reshape(B, C, H, W))
        nan = fd.clone()
        nan[1, 2, 3, 5] = float("nan")
        zeroed = want_bytes.copy()
        zeroed[1, 2, 3, 5] = 0
        od = torch.from_numpy(other).to(gpu)
        for floats, bytes_ in ((fd, want_bytes), (nan, zeroed)):
            for s in (0, 4):
                a, b = restoration_sums(floats, od, s), restoration_sums(torch.from_numpy(bytes_).to(gpu), od, s)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
                a, b = restoration_sums(od, floats, s), restoration_sums(od, torch.from_numpy(bytes_).to(gpu), s)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        want = R.image_ref(want_bytes[0], other[0], 4)
        assert np.array_equal(restoration_sums(fd, od, 4)[0][0].cpu().numpy(), R.words(want["sse"]))


def test_every_refusal_returns_without_launching(gpu):
    """ADM_EINVAL on real buffers: the sentinel-filled outputs and the ticket are as they were."""
    from adm_amd import hip
    B, C, H, W = 2, 3, 24, 24
    pred = torch.zeros(B, C, H, W, device=gpu, dtype=torch.uint8)
    f32 = torch.zeros(B * C * H * W + 1, device=gpu, dtype=torch.float32)
    sse = torch.full((B * 4 * 2 + 1,), SENTINEL, device=gpu, dtype=torch.int64)
    ssim = torch.full((B * 4 + 1,), float(SENTINEL), device=gpu, dtype=torch.float64)
    partial = torch.full((B * 4 * 2 + 1,), SENTINEL, device=gpu, dtype=torch.int64)
    ticket = torch.zeros(B + 1, device=gpu, dtype=torch.int32)
    fn = hip.lib().adm_restoration_sums
    ok = dict(pred=hip.ptr(pred), pf=0, target=hip.ptr(pred), tf=0, sse=hip.ptr(sse), ssim=hip.ptr(ssim), partial=hip.ptr(partial),
              ticket=hip.ptr(ticket), B=B, C=C, H=H, W=W, s=4)
    off = lambda t, n: hip.c_void_p(t.data_ptr() + n)
    for bad in (dict(pred=None), dict(target=None), dict(sse=None), dict(ssim=None), dict(partial=None), dict(ticket=None), dict(B=0),
                dict(B=65536), dict(C=2), dict(s=-1), dict(s=7), dict(H=18), dict(W=18), dict(H=4097, W=4096, s=0),
                dict(pred=off(f32, 2), pf=1), dict(target=off(f32, 1), tf=1), dict(sse=off(sse, 4)), dict(ssim=off(ssim, 4)),
                dict(partial=off(partial, 4)), dict(ticket=off(ticket, 2))):
        assert fn(*{**ok, **bad}.values(), hip.stream()) == -22, bad
    torch.cuda.synchronize()
    assert bool((sse == SENTINEL).all()) and bool((ssim == SENTINEL).all()) and bool((partial == SENTINEL).all()) and bool((ticket == 0).all())
    assert fn(*ok.values(), hip.stream()) == 0          # ... and the same buffers are accepted as they stand
    torch.cuda.synchronize()
    assert bool((sse[:-1] != SENTINEL).all()) and bool((ticket == 0).all())


def test_wrapper_refuses_by_name(gpu):
    from adm_amd.metrics.restoration import restoration_sums
    p = torch.zeros(2, 3, 18, 30, dtype=torch.uint8, device=gpu)
    with pytest.raises(RuntimeError, match="the target is on cpu"):
        restoration_sums(p, p.cpu())
    with pytest.raises(ValueError, match="the target must be uint8 or float32"):
        restoration_sums(p, p.double())
    with pytest.raises(ValueError, match=r"must both be \[B,C,H,W\] with C = 1 or 3"):
        restoration_sums(p, p[:, :, :, :29])
    with pytest.raises(ValueError, match=r"must both be \[B,C,H,W\] with C = 1 or 3"):
        restoration_sums(p[:, :2], p[:, :2])
    with pytest.raises(ValueError, match="a 18x30 image shaved by crop_border 4 leaves 10x22"):
        restoration_sums(p, p, 4)
    with pytest.raises(ValueError, match="crop_border must be >= 0"):
        restoration_sums(p, p, -1)
    assert restoration_sums(p, p, 3)[0].shape == (2, 4, 2)


def score_close(got, want):
    assert got["images"] == want["images"] and set(got) == set(want)
    for k in want:
        if k != "images":
            print(f"{k}: {got[k]!r} (restatement {want[k]!r})")
            assert got[k] == want[k] or abs(got[k] - want[k]) <= R.BAR, (k, got[k], want[k])


def test_score_over_two_adds_of_different_sizes_equals_the_restatement(gpu):
    from adm_amd.metrics.restoration import RestorationScore
    for C in (1, 3):
        sets = [[R.case(f, (27, 25), C) for f in ("noise", "uniform", "flat")], [R.case(f, (T + 19, 21), C, seed=1) for f in ("noise", "saturated")]]
        score = RestorationScore(4)
        for pairs in sets:
            score.add(torch.from_numpy(np.stack([p for p, _ in pairs])).to(gpu), torch.from_numpy(np.stack([g for _, g in pairs])).to(gpu))
        res = score.result()
        assert set(res) == set(R.KEYS if C == 3 else R.KEYS[:2]) | {"images"}
        score_close(res, R.dataset_ref(sets[0] + sets[1], 4))
    empty = RestorationScore().result()
    assert empty["images"] == 0 and math.isnan(empty["psnr"])


def test_eval_restoration_scores_each_pair_at_its_own_size(gpu, tmp_path):
    """Three sizes, one shared by two pairs, a JPG target paired with a PNG prediction by stem: the JSON is the restatement's on the
    decoded bytes."""
    from PIL import Image
    import eval_restoration
    pred_dir, target_dir = tmp_path / "pred", tmp_path / "target"
    pred_dir.mkdir(), target_dir.mkdir()
    pairs = []
    for i, (hw, ext) in enumerate((((40, 52), "png"), ((40, 52), "png"), ((33, 47), "jpg"), ((24, 20), "png"))):
        p, g = R.case("noise", hw, 3, seed=20 + i)
        Image.fromarray(g.transpose(1, 2, 0)).save(target_dir / f"im_{i}.{ext}")
        Image.fromarray(p.transpose(1, 2, 0)).save(pred_dir / f"im_{i}.png")
        g = np.asarray(Image.open(target_dir / f"im_{i}.{ext}").convert("RGB"), dtype=np.uint8).transpose(2, 0, 1)
        pairs.append((p, g))
    out = tmp_path / "score.json"
    res = eval_restoration.main(["--pred", str(pred_dir), "--target", str(target_dir), "--crop-border", "4", "--out_path", str(out)])
    assert json.load(open(out)) == res
    score_close(res, R.dataset_ref(pairs, 4))
    score_close(eval_restoration.main(["--pred", str(pred_dir), "--target", str(target_dir)]), R.dataset_ref(pairs, 0))


def run_sampler(cfg, tmp_path, *extra):
    path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "sample_cond_ldm.py"), "--cfg", path, "--random-init",
                        "--max-images", "1", *extra], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "PSNR: " in r.stdout and "restoration score over 1 images" in r.stdout          # the PSNR line stays
    return r.stdout


def test_sample_cond_ldm_cli_scores_the_sr_png_it_writes(gpu, tmp_path):
    """The synthetic super-resolution path at the sizes of tests/test_hip_cond_ldm.py's end-to-end run (a 94x78 image, 16x16 windows), with
    sampler.cal_restoration: True: restoration_metrics.json holds the restatement's values on the PNG's bytes against the bytes of the
    stream's target, shaved by the x4 default of 4."""
    from PIL import Image
    from sample_cond_ldm import CondStream
    cfg = yaml.load(open(os.path.join(ROOT, "configs/super-resolution/div2k_cond_ddm_const_ldm.yaml")), Loader=yaml.SafeLoader)
    cfg["model"].update(image_size=[64, 64], sampling_timesteps=2)
    cfg["model"]["first_stage"]["ddconfig"].update(ch=32, resolution=[64, 64])
    cfg["model"]["unet"].update(dim=32, class_name="unet.cond_unet_sd.Unet", window_sizes1=[[2, 2], [1, 1], [1, 1], [1, 1]],
                                window_sizes2=[[4, 4], [2, 2], [1, 1], [1, 1]])
    cfg["data"].update(image_size=[94, 78])
    out = str(tmp_path / "png")
    cfg["sampler"].update(sample_num=2, crop_size=[16, 16], stride=[8, 8], save_folder=out, cond_encoder="synthetic", window_batch=0,
                          cal_restoration=True)
    assert cfg["data"]["class_name"] == "synthetic"
    run_sampler(cfg, tmp_path)
    name = f"{0: 010d}.png"
    assert sorted(os.listdir(out)) == [name, "restoration_metrics.json"]
    png = np.asarray(Image.open(os.path.join(out, name)), dtype=np.uint8).transpose(2, 0, 1)
    assert png.shape == (3, 94, 78)
    item = next(iter(CondStream(cfg["data"], 1, gpu, seed=2000)))          # the stream the sampler's rank 0 draws from
    target = (((item["image"] + 1) * 0.5)[0, :, :94, :78].clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
    got = json.load(open(os.path.join(out, "restoration_metrics.json")))
    score_close(got, R.dataset_ref([(png, target)], 4))
    assert all(math.isfinite(got[k]) for k in R.KEYS)


def test_sample_cond_ldm_cli_scores_the_inpainting_composite_it_writes(gpu, tmp_path):
    """The in-painting sample YAML at the sizes of tests/test_hip_train_inpaint.py (128x128, a ch = 32 first stage, dim 32) on one known
    image: the composite's PNG against the image's bytes, whole (crop_border 0)."""
    from PIL import Image
    from sr_data_ref import hash_bytes
    cfg = yaml.load(open(os.path.join(ROOT, "configs/inpainting/celebahq_cond_ddm_const_ldm_sample.yaml")), Loader=yaml.SafeLoader)
    cfg["model"].update(image_size=[128, 128], sampling_timesteps=2)
    cfg["model"]["first_stage"]["ddconfig"].update(ch=32, resolution=[128, 128])
    cfg["model"]["unet"].update(dim=32, cond_feature_size=[32, 32])
    x = hash_bytes((2, 128, 128, 3), "restoration.inpaint.pool")
    np.save(tmp_path / "faces.npy", x)
    out = str(tmp_path / "png")
    cfg["data"].update(image_size=[128, 128], npy=str(tmp_path / "faces.npy"))
    cfg["sampler"].update(sample_num=2, crop_size=[128, 128], stride=[128, 128], save_folder=out, cal_restoration=True)
    run_sampler(cfg, tmp_path)
    name = f"{0: 010d}.png"
    assert sorted(os.listdir(out)) == [name, "restoration_metrics.json"]
    png = np.asarray(Image.open(os.path.join(out, name)), dtype=np.uint8).transpose(2, 0, 1)
    got = json.load(open(os.path.join(out, "restoration_metrics.json")))
    score_close(got, R.dataset_ref([(png, x[0].transpose(2, 0, 1))], 0))
    assert math.isfinite(got["psnr"]) and got["psnr"] > 0          # (the holes are the model's: not the image)
