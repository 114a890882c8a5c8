"""What tools/make_golden_kid.py and the KID tests share: the golden cases and their hash-filled features (TEST INFRASTRUCTURE ONLY).

The features are not stored: tool and tests rebuild them from ``oracle.fill.hash_tensor``.  They are Inception-like: non-negative
(a ReLU cut), about a third exact zeros, and the second set is shifted slightly so that KID comes out near 1e-2.
"""
import os
from collections import namedtuple

import torch

from oracle import fill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g30_kid.npz")
REPORT = os.path.join(ROOT, "tests", "golden", "g30_kid_report.json")

Case = namedtuple("Case", ("tag", "D", "n1", "n2", "m", "S", "degree", "gamma", "coef0"))
# gamma None = 1 / D, the reference's default.  The last case crosses a 128-row tile with a K tail (D % 32 != 0).
CASES = (
    Case("d2048", 2048, 300, 260, 128, 4, 3, None, 1.0),
    Case("d192", 192, 150, 140, 100, 3, 3, None, 1.0),
    Case("d64", 64, 80, 70, 33, 3, 3, None, 1.0),
    Case("poly2", 68, 150, 131, 129, 2, 2, 0.01, 0.5),
)
SHIFT = 0.06        # added to the second set before the cut


def features(case: Case):
    """-> (f1 [n1, D], f2 [n2, D]) float32 on the CPU"""
    out = []
    for k, n in enumerate((case.n1, case.n2)):
        u = fill.hash_tensor((n, case.D), f"kid.{case.tag}.{k}", 1.0, torch.float64)
        out.append((torch.clamp(u + 1.0 / 3.0 + k * SHIFT, min=0.0) * 1.2).float())
    return out
