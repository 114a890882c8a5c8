#!/usr/bin/env python3
"""Golden values for the saliency score: a few small prediction / map pairs with their integer tables (np.bincount) and their
per-image values and curves from the PER-PIXEL restatement (tests/saliency_ref.py), with and without normalisation.  Nothing in the
reference computes these scores; the file pins this project's own definitions (adm_amd/metrics/saliency.py) against drift.

Usage: ``python tools/make_golden_saliency.py``.  Writes tests/golden/g31_saliency.npz (the inputs themselves: they are small) and
tests/golden/g31_saliency_report.json: per case and mode the largest distance between the restatement and
``metrics_from_tables(tables_ref(...))`` -- the two independent routes to every value -- which tests/test_saliency_host.py holds to 1e-12.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import saliency_ref as R  # noqa: E402
from adm_amd.metrics import saliency as S  # noqa: E402

CASES = [("random", (7, 13)), ("saturated", (7, 13)), ("soft_block", (33, 65)), ("narrow", (5, 1)), ("one_pixel", (1, 7)),
         ("constant", (7, 13)), ("perfect", (33, 65)), ("inverted", (7, 13)), ("all_bg", (1, 1))]

g, report = {}, {}
for family, shape in CASES:
    tag = f"{family}_{shape[0]}x{shape[1]}"
    p, m = R.case(family, shape)
    tables, head = R.tables_ref(p, m)
    g[f"{tag}.pred"], g[f"{tag}.map"], g[f"{tag}.tables"], g[f"{tag}.head"] = p, m, tables, head
    report[tag] = {}
    for normalize in (True, False):
        mode = "normalized" if normalize else "raw"
        want = R.image_ref(p, m, normalize)
        got = S.per_image(tables[None], head[None], shape, normalize)
        gap = max(float(np.abs(np.asarray(got[k][0]) - want[k]).max()) for k in want)
        assert gap <= 1e-12, (tag, mode, gap)
        g[f"{tag}.{mode}.values"] = np.array([want[k] for k in ("mae", "s_measure", "adp_f", "adp_e")])
        g[f"{tag}.{mode}.f_curve"], g[f"{tag}.{mode}.e_curve"] = want["f_curve"], want["e_curve"]
        report[tag][mode] = {"mae": want["mae"], "s_measure": want["s_measure"], "adp_f": want["adp_f"], "adp_e": want["adp_e"],
                             "max_f": float(want["f_curve"].max()), "max_e": float(want["e_curve"].max()), "tables_vs_pixels": gap}
    print(tag, report[tag])

out = R.GOLDEN
np.savez_compressed(out, **g)
with open(R.REPORT, "w") as f:
    json.dump(report, f, indent=1, sort_keys=True)
assert os.path.getsize(out) < 64 * 1024, os.path.getsize(out)
print(f"wrote {out}: {os.path.getsize(out)} bytes")
