"""CPU-only: the host side of the kernel Inception distance (adm_amd/metrics/kid.py, the feature files of evaluate.py, the new flags
of eval_fid.py and ``sampler.cal_kid``).  Golden values come from the reference's own metrics.metric_kid (tools/make_golden_kid.py ->
tests/golden/g30_kid.npz); nothing here touches a GPU or a network."""
import json
import os
import re

import numpy as np
import pytest
import torch

import kid_ref as R
from adm_amd.metrics import evaluate, kid

ROOT = R.ROOT
NEW = ("adm_kid_sums", "adm_kid_sums_blocks", "adm_kid_sums_tile")


@pytest.fixture(scope="module")
def g():
    return np.load(R.GOLDEN)


def test_new_symbols_are_declared_and_bound():
    from adm_amd import hip
    header = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    declared = set(re.findall(r"^(?:int|long)\s+(adm_\w+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in declared and name in hip._SIGS, name
    assert "kid.hip" in open(os.path.join(ROOT, "adm_amd", "csrc", "Makefile")).read()
    assert "adm_kid_sums_blocks" in hip.NO_STREAM and "adm_kid_sums_tile" in hip.NO_STREAM and "adm_kid_sums" not in hip.NO_STREAM
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = hip.lib()
    for name in NEW:
        assert hasattr(lib, name), name
    # the plan: one tile form; per subset two upper triangles of T (T + 1) / 2 tiles and one square of T * T
    tile = lib.adm_kid_sums_tile(0)
    assert tile > 0 and tile % 32 == 0 and lib.adm_kid_sums_tile(1) == 0 and lib.adm_kid_sums_tile(-1) == -22
    for m, T in ((2, 1), (tile, 1), (tile + 1, 2), (1000, -(-1000 // tile))):
        assert lib.adm_kid_sums_blocks(m) == T * (T + 1) + T * T, m
    assert lib.adm_kid_sums_blocks(1) == -22


def test_arguments_outside_the_contract_return_the_error_code_without_a_launch():
    """Refusals come before any device work, so they can be asked for without a GPU (the pointers are never read)."""
    from adm_amd import hip
    lib = hip.lib()
    p = 4096          # any 16-byte aligned non-null value

    def rc(n1=10, n2=10, D=64, S=1, m=4, degree=3, f1=p):
        return lib.adm_kid_sums(f1, n1, p, n2, D, p, p, S, m, degree, 1.0, 1.0, p, p, None)
    assert rc(D=66) == -22 and rc(D=0) == -22                    # D % 4
    assert rc(m=1) == -22 and rc(m=11) == -22 and rc(n2=3) == -22      # 2 <= m <= min(n1, n2)
    assert rc(S=0) == -22
    assert rc(degree=0) == -22 and rc(degree=9) == -22
    assert rc(f1=None) == -22 and rc(f1=p + 4) == -22
    assert rc(n1=1 << 20, D=512) == -22                          # 2^31 bytes


def test_kid_indices_are_the_references_draw(g):
    for case in R.CASES:
        idx1, idx2 = kid.kid_indices(case.n1, case.n2, case.S, case.m)
        assert idx1.dtype == np.int32 and idx1.shape == (case.S, case.m)
        assert np.array_equal(idx1, g[f"{case.tag}.idx1"]) and np.array_equal(idx2, g[f"{case.tag}.idx2"]), case.tag
        assert all(len(set(row)) == case.m for row in idx1)      # without replacement
    other, _ = kid.kid_indices(R.CASES[2].n1, R.CASES[2].n2, 3, 33, rng_seed=7)
    assert not np.array_equal(other, g["d64.idx1"])


def test_mmd_from_sums_matches_the_reference(g):
    for case in R.CASES:
        got = kid.mmd_from_sums(g[f"{case.tag}.sums64"], case.m)
        want = g[f"{case.tag}.mmd64"]
        assert got.dtype == np.float64 and got.shape == (case.S,)
        print(case.tag, np.abs(got - want).max())
        assert np.all(np.abs(got - want) <= 1e-15 * np.abs(want)), case.tag
    assert torch.is_tensor(torch.from_numpy(g["d64.sums64"])) and np.array_equal(
        kid.mmd_from_sums(torch.from_numpy(g["d64.sums64"]), 33), kid.mmd_from_sums(g["d64.sums64"], 33))


def test_mean_std_and_key_names(g):
    assert kid.KEY_KID_MEAN == "kernel_inception_distance_mean" and kid.KEY_KID_STD == "kernel_inception_distance_std"
    mmds = g["d2048.mmd64"]
    res = kid.kid_from_mmds(mmds)
    assert set(res) == {kid.KEY_KID_MEAN, kid.KEY_KID_STD}
    assert res[kid.KEY_KID_MEAN] == float(np.mean(mmds)) and res[kid.KEY_KID_STD] == float(np.std(mmds))
    assert res[kid.KEY_KID_STD] == pytest.approx(np.sqrt(np.mean((mmds - mmds.mean()) ** 2)), rel=1e-12)      # ddof = 0
    report = json.load(open(R.REPORT))
    for case in R.CASES:
        # the reference's own float32 (mean, std) is within its recorded distance of the float64 values
        want32 = g[f"{case.tag}.kid32"]
        res = kid.kid_from_mmds(g[f"{case.tag}.mmd64"])
        e32 = report[case.tag]["e32"]
        assert e32 == float(np.abs(g[f"{case.tag}.mmd32"].astype(np.float64) - g[f"{case.tag}.mmd64"]).max())
        assert abs(res[kid.KEY_KID_MEAN] - want32[0]) <= e32 and abs(res[kid.KEY_KID_STD] - want32[1]) <= 2 * e32
    assert (kid.SUBSETS, kid.SUBSET_SIZE, kid.DEGREE, kid.GAMMA, kid.COEF0, kid.RNG_SEED) == (100, 1000, 3, None, 1, 2020)


def test_too_few_samples_are_refused_naming_both_counts():
    with pytest.raises(ValueError, match=r"KID subset size 1000 cannot be smaller than the number of samples \(input_1: 999, "
                                         r"input_2: 1200\)"):
        kid.kid_indices(999, 1200, 2, 1000)
    with pytest.raises(ValueError, match=r"input_1: 50, input_2: 8\)"):
        kid.kid_from_features(torch.zeros(50, 64), torch.zeros(8, 64), subsets=2, subset_size=9)
    kid.kid_indices(1000, 1000, 1, 1000)


def test_an_index_out_of_range_raises_before_any_launch(monkeypatch):
    from adm_amd import hip
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the library was reached"))
    monkeypatch.setattr(kid, "call", lambda *a: pytest.fail("a launch was reached"))
    ok = np.array([[0, 4], [3, 2]], np.int32)
    assert np.array_equal(kid.check_indices(ok, 5), ok) and kid.check_indices(ok.astype(np.int64), 5).dtype == np.int32
    with pytest.raises(IndexError, match=r"idx1\[1, 0\] = 5 is outside the 5 feature rows"):
        kid.check_indices(np.array([[0, 4], [5, 2]]), 5, "idx1")
    with pytest.raises(IndexError, match=r"idx2\[0, 1\] = -1 "):
        kid.check_indices(torch.tensor([[0, -1]]), 5, "idx2")
    with pytest.raises(ValueError, match="integer"):
        kid.check_indices(np.zeros((2, 2)), 5)
    # kid_sums makes that check before it allocates or launches anything: with the device check out of the way, it is what raises
    monkeypatch.setattr(hip, "require_cuda", lambda *a: None)
    with pytest.raises(IndexError, match=r"idx2\[0, 2\] = 7 is outside the 7 feature rows"):
        kid.kid_sums(torch.zeros(9, 8), torch.zeros(7, 8), np.array([[0, 1, 8]]), np.array([[0, 1, 7]]))


def test_cpu_features_are_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kid.kid_sums(torch.zeros(9, 8), torch.zeros(7, 8), np.array([[0, 1]]), np.array([[0, 1]]))


def test_feature_files_roundtrip_and_statistics_are_refused_by_name(tmp_path):
    from adm_amd.metrics import fid
    f = R.features(R.CASES[2])[0]
    path = str(tmp_path / "feats.npz")
    evaluate.save_features(path, f)
    with np.load(path) as z:
        assert z.files == ["features"] and z["features"].dtype == np.float32 and z["features"].shape == (80, 64)
    back = evaluate.load_features(path)
    assert back.dtype == torch.float32 and torch.equal(back, f) and evaluate.is_feature_file(path)
    evaluate.save_features(path, f.double().numpy())             # arrays too; stored as float32
    assert torch.equal(evaluate.load_features(path), f)
    stats = str(tmp_path / "target.npz")
    fid.save_stats(stats, fid.Stats(np.zeros(4), np.eye(4), 10))
    assert not evaluate.is_feature_file(stats)
    with pytest.raises(ValueError, match=r"target\.npz.*statistics hold no features"):
        evaluate.load_features(stats)
    with pytest.raises(ValueError, match="must be \\[N, D\\]"):
        evaluate.save_features(path, np.zeros(5))


def test_eval_fid_parser_accepts_the_kid_flags():
    import eval_fid
    base = ["--input1", "a", "--input2", "b", "--weights", "w"]
    a = eval_fid.build_parser().parse_args(base)
    assert not a.kid and (a.kid_subsets, a.kid_subset_size, a.kid_degree, a.kid_gamma, a.kid_coef0) == (100, 1000, 3, None, 1.0)
    assert a.save_features is None and a.save_stats is None and a.batch_size == 64
    a = eval_fid.build_parser().parse_args(base + ["--kid", "--kid-subsets", "3", "--kid-subset-size", "6", "--kid-degree", "2",
                                                   "--kid-gamma", "0.01", "--kid-coef0", "0.5", "--save-features", "x.npz", "y.npz"])
    assert a.kid and (a.kid_subsets, a.kid_subset_size, a.kid_degree, a.kid_gamma, a.kid_coef0) == (3, 6, 2, 0.01, 0.5)
    assert a.save_features == ["x.npz", "y.npz"]
    assert "--kid" in eval_fid.__doc__ and "--save-features" in eval_fid.__doc__


def test_cal_kid_makes_the_refusals_of_cal_fid(tmp_path, monkeypatch):
    import sample_uncond
    from train_uncond_dpm import Cfg
    w = tmp_path / "w.pth"
    w.write_bytes(b"placeholder")
    common = {"target_path": str(tmp_path), "save_folder": str(tmp_path / "s"), "sample_num": 4, "batch_size": 2, "cal_kid": True}
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    sample_uncond.check_cal_fid(Cfg({"sampler": dict(common, inception_weights=str(w))}))
    with pytest.raises(FileNotFoundError, match="weights file"):
        sample_uncond.check_cal_fid(Cfg({"sampler": dict(common)}))
    with pytest.raises(FileNotFoundError, match="target_path"):
        sample_uncond.check_cal_fid(Cfg({"sampler": dict(common, inception_weights=str(w), target_path=str(tmp_path / "no"))}))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        sample_uncond.check_cal_fid(Cfg({"sampler": dict(common, inception_weights=str(w))}))


def test_no_shipped_config_turns_kid_on():
    import glob
    import yaml
    for path in glob.glob(os.path.join(ROOT, "configs", "**", "*.yaml"), recursive=True):
        s = (yaml.load(open(path), Loader=yaml.SafeLoader) or {}).get("sampler") or {}
        assert not s.get("cal_kid"), path
