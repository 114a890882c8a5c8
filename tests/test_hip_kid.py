"""GPU: the kernel Inception distance on HIP (adm_amd/csrc/kid.hip, adm_amd/metrics/kid.py).

Structure, exact: the features are small integers, so every dot product is exact in float32 and every power and sum is exact in
float64; the three sums must then equal BIT FOR BIT what Python integers give, whatever the order of summation.  With gamma = 2^-g,
(gamma dot + coef0)^degree = (dot + coef0 2^g)^degree 2^(-g degree).  The test checks its own premise: the largest sum has at most 53
bits.  Accuracy: per golden case (tests/golden/g30_kid.npz, the reference's own metrics.metric_kid) each subset's MMD is within
4 e32 of the reference's float64 value, e32 being the reference's own float32 distance from that value (g30_kid_report.json).  End to
end: eval_fid.py and sample_uncond.py with the KID switches."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import inception_ref as IR
import kid_ref as R
from oracle import fill

pytestmark = pytest.mark.gpu
ROOT = R.ROOT
KID_KEYS = {"kernel_inception_distance_mean", "kernel_inception_distance_std"}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def kid():
    from adm_amd.metrics import kid
    return kid


def _tiles():
    from adm_amd import hip
    out, k = [], 0
    while hip.lib().adm_kid_sums_tile(k) > 0:
        out.append(int(hip.lib().adm_kid_sums_tile(k)))
        k += 1
    return out


# (D, n1, n2, m, S, log2(1 / gamma) or None for the default 1 / D, largest feature value)
EXACT_CASES = [
    (64, 5, 4, 2, 2, None, 3),              # the smallest legal m
    (64, 50, 45, 33, 3, None, 3),           # one row past a 32-row MFMA tile
    (64, 40, 40, 40, 1, None, 3),           # m = n: a whole permutation
    (68, 40, 37, 31, 2, 6, 3),              # the K tail
    (192, 140, 130, 129, 2, 7, 3),
    (2048, 300, 260, 128, 2, None, 1),      # features in {0, 1}
]


def _exact_cases():
    cases = list(EXACT_CASES)
    for t in _tiles():                      # every workgroup tile size the kernel has, read from the plan query
        cases += [(64, t + 9, t + 5, m, 2, None, 3) for m in (t - 1, t, t + 1)]
    return cases


def _int_features(n, D, top, tag):
    u = fill.hash_tensor((n, D), tag, 1.0, torch.float64).numpy()
    return np.minimum(np.floor((u + 1.0) * 0.5 * (top + 1)), top).astype(np.int64)


def _int_dots(a1, a2, idx1, idx2):
    """per subset the integer Gram blocks (XX, YY, XY)"""
    out = []
    for r1, r2 in zip(idx1, idx2):
        X, Y = a1[r1], a2[r2]
        out.append((X @ X.T, Y @ Y.T, X @ Y.T))
    return out


def _want(dots, g, degree, coef0):
    """-> (float64 [S, 3], the bit count of the largest integer sum)"""
    m = dots[0][0].shape[0]
    off = ~np.eye(m, dtype=bool)
    want, bits = np.zeros((len(dots), 3)), 0
    for s, (xx, yy, xy) in enumerate(dots):
        for q, (d, mask) in enumerate(((xx, off), (yy, off), (xy, None))):
            v = (d if mask is None else d[mask]).ravel().astype(object) + coef0 * (1 << g)
            total = int(np.sum(v ** degree))
            bits = max(bits, total.bit_length())
            want[s, q] = math.ldexp(float(total), -g * degree)
    return want, bits


def _tables_variant(n, m, S):
    """rows 0 and n - 1 in every subset (so rows repeat across subsets), the rest walking through the set with a stride"""
    out = np.empty((S, m), np.int32)
    for s in range(S):
        rest = [(1 + (3 * s + 5 * j) % max(n - 2, 1)) for j in range(n - 2)]
        rest = list(dict.fromkeys(rest))[:m - 2]
        out[s] = ([0, n - 1] + rest + list(range(1, n - 1)))[:m]
    return out


def test_exact_case_list_covers_every_tile_edge():
    tiles = _tiles()
    assert tiles, "the plan query names no tile"
    ms = {c[3] for c in _exact_cases()}
    for t in tiles:
        assert {t - 1, t, t + 1} <= ms


N_TILE_FORMS = 1      # the ids are fixed when the tests are collected, before the library is asked; the test below compares


@pytest.mark.parametrize("ci", range(len(EXACT_CASES) + 3 * N_TILE_FORMS))
def test_sums_are_exact_on_integer_features(gpu, kid, ci):
    cases = _exact_cases()
    assert len(_tiles()) == N_TILE_FORMS, "the kernel has another number of tile forms: set N_TILE_FORMS"
    D, n1, n2, m, S, glog, top = cases[ci]
    g = int(math.log2(D)) if glog is None else glog
    gamma = None if glog is None else 2.0 ** -glog
    assert glog is not None or 1 << g == D
    a1, a2 = _int_features(n1, D, top, f"kid.exact.{ci}.1"), _int_features(n2, D, top, f"kid.exact.{ci}.2")
    f1, f2 = torch.from_numpy(a1).float().to(gpu), torch.from_numpy(a2).float().to(gpu)
    idx1, idx2 = kid.kid_indices(n1, n2, S, m)
    dots = _int_dots(a1, a2, idx1, idx2)

    def run(i1, i2, degree, coef0):
        return kid.kid_sums(f1, f2, i1, i2, degree, gamma, coef0)

    base = run(idx1, idx2, 3, 1)
    assert base.dtype == torch.float64 and tuple(base.shape) == (S, 3) and base.is_cuda
    want, bits = _want(dots, g, 3, 1)
    assert bits <= 53, f"the premise fails: the largest sum needs {bits} bits"
    assert np.array_equal(base.cpu().numpy(), want), (base.cpu().numpy() - want)
    # the same launch again: the same bits
    assert torch.equal(run(idx1, idx2, 3, 1), base)
    for degree, coef0 in ((1, 1), (2, 1), (3, 0)):      # coef0 = 0 hides an unmasked ragged edge; the coef0 = 1 runs above do not
        want, b = _want(dots, g, degree, coef0)
        assert b <= 53
        got = run(idx1, idx2, degree, coef0).cpu().numpy()
        assert np.array_equal(got, want), (degree, coef0, got - want)
    # tables that reach row 0 and row n - 1 and repeat rows across subsets
    t1, t2 = _tables_variant(n1, m, S), _tables_variant(n2, m, S)
    assert t1.min() == 0 and t1.max() == n1 - 1 and t2.min() == 0 and t2.max() == n2 - 1
    want, b = _want(_int_dots(a1, a2, t1, t2), g, 3, 1)
    assert b <= 53
    got = run(t1, t2, 3, 1).cpu().numpy()
    assert np.array_equal(got, want), got - want
    # the MMD of exact sums, for completeness: the host half in float64
    assert np.array_equal(kid.mmd_from_sums(got, m), (want[:, 0] + want[:, 1]) / (m * (m - 1)) - 2 * want[:, 2] / (m * m))


def test_refusals_on_the_device_path(gpu, kid):
    f1, f2 = torch.zeros(9, 8, device=gpu), torch.zeros(7, 8, device=gpu)
    ok = np.array([[0, 1, 2]])
    with pytest.raises(IndexError, match=r"idx2\[0, 2\] = 7 is outside the 7 feature rows"):
        kid.kid_sums(f1, f2, ok, np.array([[0, 1, 7]]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kid.kid_sums(f1.cpu(), f2, ok, ok)
    with pytest.raises(ValueError, match="multiple of 4"):
        kid.kid_sums(torch.zeros(9, 6, device=gpu), torch.zeros(7, 6, device=gpu), ok, ok)
    with pytest.raises(ValueError, match="degree"):
        kid.kid_sums(f1, f2, ok, ok, degree=9)
    with pytest.raises(ValueError, match="subset size"):
        kid.kid_sums(f1, f2, np.array([[0]]), np.array([[0]]))
    assert tuple(kid.kid_sums(f1, f2, ok, ok).shape) == (1, 3)


@pytest.mark.parametrize("case", R.CASES, ids=[c.tag for c in R.CASES])
def test_mmd_against_the_reference_in_float64(gpu, kid, case):
    g, report = np.load(R.GOLDEN), json.load(open(R.REPORT))
    e32 = report[case.tag]["e32"]
    assert e32 == float(np.abs(g[f"{case.tag}.mmd32"].astype(np.float64) - g[f"{case.tag}.mmd64"]).max()) and 0 < e32 < 1e-5
    f1, f2 = (f.to(gpu) for f in R.features(case))
    idx1, idx2 = kid.kid_indices(case.n1, case.n2, case.S, case.m)
    assert np.array_equal(idx1, g[f"{case.tag}.idx1"]) and np.array_equal(idx2, g[f"{case.tag}.idx2"])
    sums = kid.kid_sums(f1, f2, idx1, idx2, case.degree, case.gamma, case.coef0).cpu().numpy()
    mmd = kid.mmd_from_sums(sums, case.m)
    d_mmd = float(np.abs(mmd - g[f"{case.tag}.mmd64"]).max())
    d_sum = float(np.abs(sums - g[f"{case.tag}.sums64"]).max())
    # a sum moves the MMD by d / (m (m - 1)) (XX, YY) or 2 d / m^2 (XY): an error of e32 m^2 / 2 in one sum is an error of e32 there
    sum_bar = e32 * case.m ** 2 / 2
    print(f"{case.tag}: |mmd - mmd64| = {d_mmd:.3e} = {d_mmd / e32:.4f} e32 (bar 4); |sums - sums64| = {d_sum:.3e} = "
          f"{d_sum / sum_bar:.4f} of e32 m^2 / 2 (bar 4); e32 = {e32:.3e}")
    assert d_mmd <= 4 * e32
    assert d_sum <= 4 * sum_bar
    res = kid.kid_from_features(f1, f2, case.S, case.m, case.degree, case.gamma, case.coef0)
    assert res == kid.kid_from_mmds(mmd)


@pytest.fixture(scope="module")
def weights_file(tmp_path_factory):
    from adm_amd.metrics import inception
    path = str(tmp_path_factory.mktemp("inception") / "synthetic_inception.pth")
    torch.save(IR.synthetic_state_dict(inception.state_dict_shapes()), path)
    return path


def _write_pngs(folder, imgs):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for i, a in enumerate(imgs.permute(0, 2, 3, 1).numpy()):
        Image.fromarray(a).save(os.path.join(folder, f"{i: 010d}.png"))


def test_cli_eval_fid_with_kid(gpu, kid, weights_file, tmp_path, capsys):
    import eval_fid
    from adm_amd.metrics import evaluate
    a, b = (s[:8] for s in IR.e2e_sets())
    _write_pngs(str(tmp_path / "a"), a)
    _write_pngs(str(tmp_path / "b"), b)
    fa, fb, out = str(tmp_path / "fa.npz"), str(tmp_path / "fb.npz"), str(tmp_path / "out" / "result.json")
    flags = ["--weights", weights_file, "--batch-size", "8", "--kid", "--kid-subsets", "3", "--kid-subset-size", "6"]
    res = eval_fid.main(["--input1", str(tmp_path / "a"), "--input2", str(tmp_path / "b"), "--out_path", out,
                         "--save-features", fa, fb] + flags)
    assert set(res) == KID_KEYS | {"frechet_inception_distance"} and json.load(open(out)) == res
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
    assert all(np.isfinite(v) for v in res.values()) and res["kernel_inception_distance_std"] > 0
    f1, f2 = evaluate.load_features(fa), evaluate.load_features(fb)
    assert tuple(f1.shape) == tuple(f2.shape) == (8, 2048) and float(f1.abs().max()) > 0 and not torch.equal(f1, f2)
    want = kid.kid_from_features(f1.to(gpu), f2.to(gpu), subsets=3, subset_size=6)
    assert {k: res[k] for k in KID_KEYS} == want
    # from the two saved feature files: the same KID bit for bit, the FID from statistics streamed from the features
    again = eval_fid.main(["--input1", fa, "--input2", fb] + flags)
    assert {k: again[k] for k in KID_KEYS} == want
    assert again["frechet_inception_distance"] == pytest.approx(res["frechet_inception_distance"], rel=1e-9)
    # statistics hold no features
    stats = str(tmp_path / "a_stats.npz")
    evaluate.save_stats(stats, evaluate.Stats(np.zeros(2048), np.eye(2048), 8))
    with pytest.raises(ValueError, match=r"a_stats\.npz.*statistics hold no features"):
        eval_fid.main(["--input1", fa, "--input2", stats] + flags)


def test_cli_sample_uncond_with_cal_kid(gpu, weights_file, tmp_path):
    cfg = yaml.load(open(os.path.join(ROOT, "configs", "cifar10", "ddm_uncond_const_uncond_unet.yaml")), Loader=yaml.SafeLoader)
    cfg["model"]["unet"].update(model_channels=64, num_blocks=1)
    target, res = str(tmp_path / "target"), str(tmp_path / "run")
    _write_pngs(target, IR.e2e_sets()[1][:8])
    cfg["sampler"].update(batch_size=8, sample_num=8, save_folder=os.path.join(res, "png"), target_path=target,
                          inception_weights=weights_file, cal_kid=True, kid_subsets=3, kid_subset_size=6)
    path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sample_uncond.py"), "--cfg", path, "--random-init", "--max-batches", "1"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(os.path.join(res, "png"))) == sorted([f"{i: 010d}.png" for i in range(8)] + ["result.json"])
    out = json.load(open(os.path.join(res, "png", "result.json")))
    assert set(out) == KID_KEYS and all(np.isfinite(v) for v in out.values())
    assert os.path.isfile(target + ".features.npz") and not os.path.exists(target + ".npz")
