#!/usr/bin/env python3
"""Golden values for the restoration score: a few small prediction / target pairs with the sums the kernel makes (the two SSE words
and the float64 sum of each plane's SSIM map) and their metrics, all from the per-image restatement with the DIRECT 2-D window
(tests/restoration_ref.py).  Nothing in the reference computes these scores; the file pins this project's own definitions
(adm_amd/metrics/restoration.py) against drift.  Runs on the CPU.

Usage: ``python tools/make_golden_restoration.py``.  Writes tests/golden/g32_restoration.npz (the inputs themselves: they are small) and
tests/golden/g32_restoration_report.json: per case the metrics and the largest per-plane SSIM distance of the restatement from
scipy.signal.convolve2d(..., 'valid') with the same window, from the separable float64 filter (the kernel's order of operations) and
from the separable float32 filter (the defect the 1e-10 bar is there to reject); tests/test_restoration_host.py holds the first two to
the bar and the flat pair's float32 distance above it.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import restoration_ref as R  # noqa: E402
from adm_amd.metrics import restoration as M  # noqa: E402

# (family, (H, W), C, crop_border)
CASES = [("uniform", (19, 23), 3, 4), ("uniform", (11, 12), 1, 0), ("saturated", (21, 20), 3, 0), ("equal", (12, 11), 3, 0),
         ("flat", (24, 24), 3, 0), ("flat", (19, 21), 1, 4), ("noise", (27, 25), 3, 4), ("noise", (13, 17), 1, 0), ("fringe", (23, 22), 3, 0)]

g, report = {}, {}
for family, shape, C, s in CASES:
    tag = f"{family}_{shape[0]}x{shape[1]}_c{C}_s{s}"
    p, t = R.case(family, shape, C)
    want = R.image_ref(p, t, s)
    Hs, Ws = shape[0] - 2 * s, shape[1] - 2 * s
    sums = want["ssim_planes"] * ((Hs - R.K + 1) * (Ws - R.K + 1))
    got = M.per_image(R.words(want["sse"])[None], sums[None], (Hs, Ws))
    keys = [k for k in R.KEYS if k in want]
    for k in keys:
        assert got[k][0] == want[k] or abs(got[k][0] - want[k]) <= 1e-12, (tag, k, got[k][0], want[k])
    gaps = {}
    for name, fn in (("vs_scipy_convolve2d", R.ssim_scipy), ("vs_separable_float64", R.ssim_separable),
                     ("vs_separable_float32", lambda a, b: R.ssim_separable(a, b, np.float32).astype(np.float64))):
        other = R.image_ref(p, t, s, ssim=fn)
        gaps[name] = float(np.abs(other["ssim_planes"] - want["ssim_planes"]).max())
    assert gaps["vs_scipy_convolve2d"] <= R.BAR and gaps["vs_separable_float64"] <= R.BAR, (tag, gaps)
    g[f"{tag}.pred"], g[f"{tag}.target"] = p, t
    g[f"{tag}.sse"], g[f"{tag}.ssim_sum"] = R.words(want["sse"]), sums
    g[f"{tag}.values"] = np.array([want[k] for k in keys])
    report[tag] = dict({k: (want[k] if np.isfinite(want[k]) else "inf") for k in keys}, sse=[str(v) for v in want["sse"]], **gaps)
    print(tag, report[tag])

np.savez_compressed(R.GOLDEN, **g)
with open(R.REPORT, "w") as f:
    json.dump(report, f, indent=1, sort_keys=True)
    f.write("\n")
assert os.path.getsize(R.GOLDEN) < 64 * 1024, os.path.getsize(R.GOLDEN)
print(f"wrote {R.GOLDEN}: {os.path.getsize(R.GOLDEN)} bytes")
