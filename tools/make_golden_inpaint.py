#!/usr/bin/env python3
"""Golden vectors for the in-painting masks: the reference's own ddm/data.py run on SCRIPTED draws.  RUNS ONLY IN THE BUILD
CONTAINER (needs /root/reference and PIL; no GPU).  ddm.data is imported with stub modules for what is not installed (torchvision,
albumentations); its ``np`` is replaced by a proxy whose ``random`` answers every call of InpaintDataset.random_mask / RandomBrush
(ddm/data.py:404-476) from the fixed slot table of include/adm_hip.h, in call order, so the reference's own rejection loop consumes
the candidate slabs one after another.  ``ImageDraw`` and ``RandomBrush`` are wrapped to record what the reference drew.

Writes tests/golden/g22_inpaint.npz --
  s{64,256}.u / .z             the draws, float32 [64, 4, NU] / [64, 4, NZ]
  s*.chosen                    candidates the reference's loop consumed, minus one
  s*.raw_rects / .rect_drawn   the (x, y, w, h) the script handed to Fill, by slot
  s*.verts / .nverts / .widths what the reference passed to ImageDraw.line
  s*.flips                     its two final flips
  s*.mask / s*.brush           its masks (random_mask's result; RandomBrush's return value alone), bit-packed
  hand{64,256}.*               hand-placed primitive lists rendered by PIL through the same calls
  stat.*                       hole ratio of 4096 masks of the UNPATCHED reference under a fixed numpy seed
-- and tests/golden/g22_inpaint_report.json: the measured band and mismatch share of the integer restatement (tests/inpaint_ref.py)
against those masks."""
import json
import os
import sys
import types

import numpy as np
import PIL
from PIL import Image, ImageDraw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)


class _Meta(type):
    def __getattr__(cls, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return cls()


class _Stub(metaclass=_Meta):
    """import-time placeholder: any attribute exists; an instance applied to a function returns the function"""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return a[0] if (len(a) == 1 and callable(a[0]) and not k) else self

    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return _Stub()


class _StubModule(types.ModuleType):
    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return _Stub


for name in ["torchvision", "torchvision.transforms", "torchvision.transforms.functional", "torchvision.datasets", "albumentations"]:
    m = _StubModule(name); m.__path__ = []; sys.modules[name] = m

import ddm.data as D  # noqa: E402  (the reference's)

import inpaint_ref as R  # noqa: E402
from adm_amd.ddm import inpaint_data as T  # noqa: E402

K = T.CANDIDATES
BAND_LIMIT, SHARE_LIMIT = 1.5, 0.02


class ScriptedRandom:
    """np.random for one sample: every call is answered from slab k of u [K, NU] / z [K, NZ]; a candidate that ends (its second flip
    draw was consumed) is followed by slab k + 1."""

    def __init__(self, u, z):
        self.u, self.z, self.k, self.log = u, z, -1, None
        self.plan, self.req = None, None

    def _calls(self):
        """The slots of one candidate in the reference's call order; receives each answered value."""
        n = yield ("u", T.U_NRECT_SMALL)
        for j in range(n):
            for c in range(4):
                yield ("u", T.U_RECT + 4 * j + c)
        n = yield ("u", T.U_NRECT_BIG)
        for c in range(4 * n):
            yield ("u", T.U_RECT + 4 * (T.RECTS - 1) + c)
        n = yield ("u", T.U_NSTROKE)
        for s in range(n):
            base = T.U_STROKE + s * T.STROKE_U
            nv = yield ("u", base + T.S_NUM_VERTEX)
            yield ("u", base + T.S_ANGLE_MIN)
            yield ("u", base + T.S_ANGLE_MAX)
            for i in range(nv):
                yield ("u", base + T.S_ANGLES + i)
            yield ("u", base + T.S_START)
            yield ("u", base + T.S_START + 1)
            for i in range(nv):
                yield ("z", s * T.SEGMENTS + i)
            yield ("u", base + T.S_WIDTH)
            yield ("u", base + T.S_DISCARD)
            yield ("u", base + T.S_DISCARD + 1)
        yield ("u", T.U_FLIP)
        yield ("u", T.U_FLIP + 1)

    def _answer(self, kind, fn):
        if self.plan is None:
            self.k += 1
            assert self.k < K, "the reference asked for more candidates than the slot table holds"
            self.plan, self.log = self._calls(), {}
            self.req = next(self.plan)
        want, slot = self.req
        assert want == kind, f"call order: the script expected a {want} draw at slot {slot}"
        v = fn(float(self.u[self.k, slot]) if kind == "u" else float(self.z[self.k, slot]))
        self.log[(kind, slot)] = v
        try:
            self.req = self.plan.send(v)
        except StopIteration:
            self.plan = None
        return v

    def randint(self, lo, hi=None):
        if hi is None:
            lo, hi = 0, lo
        return self._answer("u", lambda u: R.randint(u, lo, hi))

    def uniform(self, a, b):
        return self._answer("u", lambda u: R.uniform(u, a, b))

    def random(self):
        return self._answer("u", lambda u: u)

    def normal(self, loc, scale):
        return self._answer("z", lambda z: loc + scale * z)


class NumpyProxy:
    def __init__(self, random):
        self.random = random

    def __getattr__(self, n):
        return getattr(np, n)


class Recorder:
    """Stands for the module's ImageDraw and RandomBrush: records the line calls and the brush mask of the LAST RandomBrush call (the
    accepted candidate)."""

    def __init__(self):
        self.brush_fn = D.RandomBrush
        self.lines, self.brush = [], None

    def Draw(self, im):          # ImageDraw.Draw
        rec, real = self, ImageDraw.Draw(im)

        class _Draw:
            def line(self, xy, fill=None, width=0):
                rec.lines.append(([(int(x), int(y)) for x, y in xy], int(width)))
                return real.line(xy, fill=fill, width=width)

            def ellipse(self, *a, **k):
                return real.ellipse(*a, **k)
        return _Draw()

    def RandomBrush(self, *a, **k):
        self.lines = []
        self.brush = np.array(self.brush_fn(*a, **k), dtype=np.uint8)
        return self.brush


def reference_sample(u, z, S):
    """The reference's random_mask on one sample's script -> (chosen, candidate as the reference saw it, mask, brush)."""
    src, rec = ScriptedRandom(u, z), Recorder()
    saved = D.np, D.ImageDraw, D.RandomBrush
    D.np, D.ImageDraw, D.RandomBrush = NumpyProxy(src), rec, rec.RandomBrush
    try:
        mask = D.InpaintDataset.random_mask(None, S, hole_range=[0, 1])
    finally:
        D.np, D.ImageDraw, D.RandomBrush = saved
    assert src.plan is None and mask.shape == (1, S, S) and mask.dtype == np.float32
    log = src.log
    rects = [(j,) + tuple(log[("u", T.U_RECT + 4 * j + c)] for c in (2, 3, 0, 1)) for j in range(log[("u", T.U_NRECT_SMALL)])]
    if log[("u", T.U_NRECT_BIG)]:
        j = T.RECTS - 1
        rects.append((j,) + tuple(log[("u", T.U_RECT + 4 * j + c)] for c in (2, 3, 0, 1)))
    cand = {"raw_rects": rects, "strokes": list(rec.lines),
            "flips": (int(log[("u", T.U_FLIP)] > 0.5), int(log[("u", T.U_FLIP + 1)] > 0.5))}
    assert len(cand["strokes"]) == log[("u", T.U_NSTROKE)]
    return src.k, cand, mask[0].astype(np.uint8), rec.brush


def script(S, B, seed):
    """Draws as torch makes them (float32 in [0, 1) / N(0, 1)), with a few slabs forced empty so the rejection loop shows: sample 0's
    first three candidates and sample 1's first (a drawn rectangle of width 0) cover nothing."""
    rng = np.random.default_rng(seed)
    u = rng.random((B, K, T.NU), dtype=np.float32)
    z = rng.standard_normal((B, K, T.NZ), dtype=np.float32)
    for k in range(3):
        u[0, k, [T.U_NRECT_SMALL, T.U_NRECT_BIG, T.U_NSTROKE]] = 0.0
    u[1, 0, [T.U_NRECT_BIG, T.U_NSTROKE]] = 0.0
    u[1, 0, T.U_NRECT_SMALL], u[1, 0, T.U_RECT] = 0.3, 0.0          # one small rectangle, w = 0
    u[0, 3, T.U_NSTROKE], u[1, 1, T.U_NSTROKE] = 0.9, 0.5           # the candidates that end the two loops are not empty
    return u, z


def pil_render(c, S):
    """A hand-placed candidate through the calls the reference makes (data.py:407-418, 435-476) -> (mask, brush)."""
    mask = np.ones((S, S), np.uint8)
    for _, x, y, w, h in c["raw_rects"]:
        mask[max(y, 0): min(y + h, S), max(x, 0): min(x + w, S)] = 0
    im = Image.new("L", (S, S), 0)
    for vertex, width in c["strokes"]:
        draw = ImageDraw.Draw(im)
        draw.line(vertex, fill=1, width=width)
        for v in vertex:
            draw.ellipse((v[0] - width // 2, v[1] - width // 2, v[0] + width // 2, v[1] + width // 2), fill=1)
    brush = np.asarray(im, np.uint8)
    if c["flips"][0]:
        brush = np.flip(brush, 0)
    if c["flips"][1]:
        brush = np.flip(brush, 1)
    mask = np.logical_and(mask, 1 - brush)
    return mask.astype(np.uint8), np.ascontiguousarray(brush)


def zigzag(n, S, x0, y0, step):
    return [(min(max(x0 + i * step, 0), S), min(max(y0 + (i % 2) * step * 2 + (i // 4) * 3, 0), S)) for i in range(n)]


def hand_cases():
    """{S: [(name, candidate)]}"""
    s = 64
    asym = {"raw_rects": [(0, 3, 40, 20, 9)], "strokes": [([(10, 8), (30, 14), (50, 30), (44, 52), (20, 40)], 12)]}
    c64 = [
        ("corner", {"raw_rects": [], "strokes": [([(40, 44), (s, s), (52, s), (s, 50), (s, s)], 12)], "flips": (0, 0)}),
        ("repeat", {"raw_rects": [], "strokes": [([(8, 8), (20, 30), (20, 30), (50, 34), (50, 34)], 13)], "flips": (0, 0)}),
        ("v18", {"raw_rects": [], "strokes": [(zigzag(18, s, 2, 4, 4), 12)], "flips": (0, 0)}),
        ("w12", {"raw_rects": [], "strokes": [([(0, 10), (31, 23), (s, 12), (33, 50), (5, 60)], 12)], "flips": (0, 0)}),
        ("w47", {"raw_rects": [], "strokes": [([(4, 4), (12, 9), (9, 20), (3, 12), (0, 0)], 47)], "flips": (0, 0)}),
        ("rect_left", {"raw_rects": [(0, -5, 10, 12, 9)], "strokes": [], "flips": (0, 0)}),
        ("rect_top", {"raw_rects": [(1, 20, -4, 9, 11)], "strokes": [], "flips": (0, 0)}),
        ("rect_right", {"raw_rects": [(2, 57, 30, 16, 8)], "strokes": [], "flips": (0, 0)}),
        ("rect_bottom", {"raw_rects": [(3, 11, 50, 40, 31)], "strokes": [], "flips": (0, 0)}),
        ("rect_outside", {"raw_rects": [(0, s + 5, s + 2, 9, 9), (1, 30, 31, 4, 5)], "strokes": [], "flips": (0, 0)}),
    ]
    c64 += [(f"flip{a}{b}", dict(asym, flips=(a, b))) for a in (0, 1) for b in (0, 1)]
    S = 256
    full = {"raw_rects": [(0, -10, 30, 60, 90), (1, 100, -20, 127, 50), (2, 200, 180, 100, 100), (3, 40, 150, 200, 255)],
            "strokes": [(zigzag(18, S, 5 + 30 * k, 8 + 33 * k, 13 - k), 12 + 5 * k) for k in range(7)], "flips": (1, 0)}
    return {64: c64, 256: [("full", full)]}


def pack_reference(cands, S):
    p = R.pack(cands, S)
    B = len(cands)
    raw, drawn = np.zeros((B, T.RECTS, 4), np.int32), np.zeros((B, T.RECTS), np.uint8)
    for b, c in enumerate(cands):
        for j, x, y, w, h in c["raw_rects"]:
            raw[b, j], drawn[b, j] = (x, y, w, h), 1
    return {"raw_rects": raw, "rect_drawn": drawn, "verts": p["verts"], "nverts": p["nverts"], "widths": p["widths"], "flips": p["flips"]}


def main():
    g = {"pil_version": np.array(PIL.__version__)}
    report = {"pil": PIL.__version__, "numpy": np.__version__, "band_limit_px": BAND_LIMIT, "share_limit": SHARE_LIMIT, "sets": {}}
    tot = [0.0, 0, 0]
    for S, seed in ((64, 6401), (256, 25601)):
        u, z = script(S, 64, seed)
        runs = [reference_sample(u[b], z[b], S) for b in range(u.shape[0])]
        # The reference also redraws a candidate whose every pixel is a hole (ratio 1: wide strokes on a small image); the kernel does
        # not.  Such a sample is given fresh draws, and the report says how many were.
        rng, full = np.random.default_rng(seed + 1), 0
        for b in range(u.shape[0]):
            while runs[b][0] != R.geometry(u[b], z[b], S)[0]:
                full += 1
                u[b], z[b] = rng.random((K, T.NU), dtype=np.float32), rng.standard_normal((K, T.NZ), dtype=np.float32)
                runs[b] = reference_sample(u[b], z[b], S)
        cands = [r[1] for r in runs]
        masks, brush = np.stack([r[2] for r in runs]), np.stack([r[3] for r in runs])
        g[f"s{S}.u"], g[f"s{S}.z"] = u, z
        g[f"s{S}.chosen"] = np.array([r[0] for r in runs], np.int32)
        for k, v in pack_reference(cands, S).items():
            g[f"s{S}.{k}"] = v
        g[f"s{S}.mask"], g[f"s{S}.brush"] = np.packbits(masks, axis=-1), np.packbits(brush, axis=-1)
        # the restatement against what the reference did
        ours, fell = R.geometry_batch(u, z, S)
        assert fell == 0 and np.array_equal(ours["chosen"], g[f"s{S}.chosen"])
        ref = R.pack(cands, S)
        assert all(np.array_equal(ours[k], ref[k]) for k in ("rects", "verts", "nverts", "widths", "flips")), "geometry differs"
        mine = R.raster_batch(ours, S)
        no_stroke = [b for b, c in enumerate(cands) if not c["strokes"]]
        assert all(np.array_equal(mine[b], masks[b]) for b in no_stroke), "a rectangle-only mask differs"
        band, differ, covered = R.compare_strokes(cands, brush, S)
        report["sets"][f"s{S}"] = {"samples": len(cands), "strokes": sum(len(c["strokes"]) for c in cands), "rect_only_samples": len(no_stroke),
                                   "samples_redrawn_for_a_full_hole_candidate": full,
                                   "chosen_histogram": np.bincount(g[f"s{S}.chosen"], minlength=K).tolist(), "band_px": band,
                                   "differing_pixels": differ, "pil_covered_pixels": covered, "share": differ / covered}
        tot = [max(tot[0], band), tot[1] + differ, tot[2] + covered]
    for S, cases in hand_cases().items():
        cands = [c for _, c in cases]
        rendered = [pil_render(c, S) for c in cands]
        masks, brush = np.stack([r[0] for r in rendered]), np.stack([r[1] for r in rendered])
        g[f"hand{S}.names"] = np.array([n for n, _ in cases])
        for k, v in pack_reference(cands, S).items():
            g[f"hand{S}.{k}"] = v
        g[f"hand{S}.mask"], g[f"hand{S}.brush"] = np.packbits(masks, axis=-1), np.packbits(brush, axis=-1)
        mine = R.raster_batch(R.pack(cands, S), S)
        for (n, c), a, m in zip(cases, mine, masks):
            assert c["strokes"] or np.array_equal(a, m), f"hand case {n}: a rectangle-only mask differs"
        band, differ, covered = R.compare_strokes(cands, brush, S)
        report["sets"][f"hand{S}"] = {"cases": [n for n, _ in cases], "band_px": band, "differing_pixels": differ,
                                      "pil_covered_pixels": covered, "share": differ / covered}
        tot = [max(tot[0], band), tot[1] + differ, tot[2] + covered]
    report["fixture"] = {"band_px": tot[0], "differing_pixels": tot[1], "pil_covered_pixels": tot[2], "share": tot[1] / tot[2]}
    assert tot[0] <= BAND_LIMIT and tot[1] / tot[2] <= SHARE_LIMIT, report["fixture"]

    # the statistical pin: the unpatched reference under numpy's own generator
    S, N, seed = 64, 4096, 20240607
    np.random.seed(seed)
    ratio = np.array([1.0 - float(D.InpaintDataset.random_mask(None, S, hole_range=[0, 1]).mean()) for _ in range(N)])
    g["stat.size"], g["stat.n"], g["stat.seed"] = np.array(S), np.array(N), np.array(seed)
    g["stat.mean"], g["stat.std"] = np.array(ratio.mean()), np.array(ratio.std(ddof=1))
    report["hole_ratio"] = {"size": S, "masks": N, "numpy_seed": seed, "mean": float(ratio.mean()), "std": float(ratio.std(ddof=1))}

    out = os.path.join(ROOT, "tests", "golden", "g22_inpaint.npz")
    np.savez_compressed(out, **g)
    with open(os.path.join(ROOT, "tests", "golden", "g22_inpaint_report.json"), "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(f"wrote {out}: {os.path.getsize(out)} bytes")
    print(json.dumps(report["fixture"]), json.dumps(report["hole_ratio"]))


if __name__ == "__main__":
    main()
