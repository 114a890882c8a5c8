#!/usr/bin/env python3
"""Golden values for the kernel Inception distance: the reference's own ``metrics.metric_kid`` (torch-fidelity, vendored under
metrics/ of the reference checkout) run on the CPU.  Usage: ``python tools/make_golden_kid.py <reference checkout>``.

metrics.utils imports torchvision and metric_kid imports tqdm, neither a dependency here: stub modules in sys.modules are enough,
nothing of them is called (the tool passes ``verbose=False``).

Writes tests/golden/g30_kid.npz and tests/golden/g30_kid_report.json.  The features are NOT stored: tests/kid_ref.py rebuilds them
from ``oracle.fill.hash_tensor``.  Per case of ``kid_ref.CASES`` the file holds
  idx1 / idx2  the subsets ``kid_features_to_metric`` drew, recorded from its own calls of ``polynomial_mmd`` (the rows it passed are
               looked up in the feature matrices; the rows are pairwise distinct)
  mmd32        what those calls returned: the reference's float32 result, per subset; kid32 = the (mean, std) it reported
  sums64       sum_{i != j} K_XX, sum_{i != j} K_YY, sum K_XY per subset from the reference's ``polynomial_kernel`` on the float64 cast
               of the same rows, added in ``mmd2``'s order; mmd64 = its ``mmd2`` of those three matrices
and the report holds e32 = max over the subsets of |mmd32 - mmd64|: the reference's own float32 distance from the float64 value,
which the GPU tests use as their yardstick (tests/test_hip_kid.py).  ``measured_on_gpu`` is filled in by hand from that test's output.
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.path.abspath(sys.argv[1])
sys.path.insert(1, REF)
for stub in ("torchvision", "torchvision.transforms", "torchvision.datasets", "torchvision.transforms.functional", "tqdm"):
    if stub not in sys.modules:
        try:
            __import__(stub)
        except ImportError:
            m = types.ModuleType(stub)
            m.__path__ = []

            def _any(name):                                       # any plain attribute is an empty class: enough for imports
                if name.startswith("__"):
                    raise AttributeError(name)
                return type(name, (), {})
            m.__getattr__ = _any
            m.tqdm = lambda it=None, **k: it
            sys.modules[stub] = m

import kid_ref as R  # noqa: E402
from metrics import metric_kid  # noqa: E402
from metrics.metric_kid import kid_features_to_metric, mmd2, polynomial_kernel  # noqa: E402


def row_lookup(f):
    table = {row.tobytes(): i for i, row in enumerate(f)}
    assert len(table) == len(f), "two equal feature rows: change the fill"
    return table


g, report = {}, {}
try:                                          # figures copied in by hand survive a re-run that changes nothing else
    kept = {k: v.get("measured_on_gpu") for k, v in json.load(open(R.REPORT)).items()}
except (OSError, ValueError):
    kept = {}
for case in R.CASES:
    f1, f2 = R.features(case)
    a1, a2 = f1.numpy(), f2.numpy()
    assert a1.dtype == np.float32 and a1.min() >= 0 and a2.min() >= 0
    zeros = float((a1 == 0).mean())
    assert 0.25 <= zeros <= 0.4, zeros
    look1, look2 = row_lookup(a1), row_lookup(a2)

    calls = []
    inner = metric_kid.polynomial_mmd

    def recording(x, y, degree, gamma, coef0):
        out = inner(x, y, degree, gamma, coef0)
        calls.append(([look1[r.tobytes()] for r in x], [look2[r.tobytes()] for r in y], out))
        return out
    metric_kid.polynomial_mmd = recording
    try:
        res32 = kid_features_to_metric(f1, f2, kid_subsets=case.S, kid_subset_size=case.m, kid_degree=case.degree,
                                       kid_gamma=case.gamma, kid_coef0=case.coef0, verbose=False)
    finally:
        metric_kid.polynomial_mmd = inner
    assert len(calls) == case.S
    idx1 = np.array([c[0] for c in calls], np.int32)
    idx2 = np.array([c[1] for c in calls], np.int32)
    mmd32 = np.array([c[2] for c in calls])
    assert mmd32.dtype == np.float32, mmd32.dtype
    assert idx1.shape == idx2.shape == (case.S, case.m)

    sums64, mmd64 = np.zeros((case.S, 3)), np.zeros(case.S)
    for s in range(case.S):
        X, Y = a1[idx1[s]].astype(np.float64), a2[idx2[s]].astype(np.float64)
        kxx = polynomial_kernel(X, X, degree=case.degree, gamma=case.gamma, coef0=case.coef0)
        kyy = polynomial_kernel(Y, Y, degree=case.degree, gamma=case.gamma, coef0=case.coef0)
        kxy = polynomial_kernel(X, Y, degree=case.degree, gamma=case.gamma, coef0=case.coef0)
        assert kxx.dtype == np.float64
        # added up in mmd2's own order (row sums less the diagonal, then their sum; column sums, then their sum), so that the
        # recorded sums and the recorded MMD are one computation
        sums64[s] = [(kxx.sum(axis=1) - np.diagonal(kxx)).sum(), (kyy.sum(axis=1) - np.diagonal(kyy)).sum(), kxy.sum(axis=0).sum()]
        mmd64[s] = mmd2(kxx, kxy, kyy)
    e32 = float(np.abs(mmd32.astype(np.float64) - mmd64).max())
    assert e32 > 0
    g[f"{case.tag}.idx1"], g[f"{case.tag}.idx2"] = idx1, idx2
    g[f"{case.tag}.sums64"], g[f"{case.tag}.mmd64"], g[f"{case.tag}.mmd32"] = sums64, mmd64, mmd32
    g[f"{case.tag}.kid32"] = np.array([res32["kernel_inception_distance_mean"], res32["kernel_inception_distance_std"]])
    report[case.tag] = {"shape": list(case[1:6]), "degree": case.degree, "gamma": case.gamma, "coef0": case.coef0,
                        "zero_share": zeros, "kid64_mean": float(mmd64.mean()), "kid64_std": float(mmd64.std()),
                        "kid32_mean": res32["kernel_inception_distance_mean"], "e32": e32, "measured_on_gpu": kept.get(case.tag)}
    print(case.tag, report[case.tag])

out = os.path.join(ROOT, "tests", "golden", "g30_kid.npz")
np.savez_compressed(out, **g)
with open(os.path.join(ROOT, "tests", "golden", "g30_kid_report.json"), "w") as f:
    json.dump(report, f, indent=1, sort_keys=True)
assert os.path.getsize(out) < (1 << 20), out
print(f"wrote {out}: {os.path.getsize(out)} bytes")
