"""CPU: the in-painting masks' definition (tests/inpaint_ref.py, the NumPy restatement of adm_amd/csrc/inpaint_data.hip) against the
reference's own run recorded in tests/golden/g22_inpaint.npz (tools/make_golden_inpaint.py: ddm/data.py on scripted draws, PIL
12.2.0), and the host half of adm_amd/ddm/inpaint_data.py.

Geometry and rectangles are exact: zero differences.  Strokes are matched up to PIL's boundary rounding: every pixel that differs
from PIL's rendering lies within BAND px of the analytic boundary and the differing pixels are at most SHARE of PIL's covered
pixels (the bounds of the issue that defined the mask; measured when the golden was made: 1.42 px as an upper bound on a 0.01 px
ladder, 0.74 %)."""
import json
import os
import re

import numpy as np
import pytest
import torch

import inpaint_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "g22_inpaint.npz")
REPORT = os.path.join(HERE, "golden", "g22_inpaint_report.json")
BAND, SHARE = 1.5, 0.02
SETS = (("s64", 64), ("s256", 256), ("hand64", 64), ("hand256", 256))


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def reference_cands(g, tag):
    """The golden's lists as candidates (what R.pack takes)."""
    out = []
    for b in range(g[f"{tag}.nverts"].shape[0]):
        rects = [(j,) + tuple(int(v) for v in g[f"{tag}.raw_rects"][b, j]) for j in range(R.RECTS) if g[f"{tag}.rect_drawn"][b, j]]
        strokes = [([tuple(int(c) for c in v) for v in g[f"{tag}.verts"][b, s, :n]], int(g[f"{tag}.widths"][b, s]))
                   for s, n in enumerate(g[f"{tag}.nverts"][b]) if n]
        out.append({"raw_rects": rects, "strokes": strokes, "flips": tuple(int(f) for f in g[f"{tag}.flips"][b])})
    return out


def unpack(g, key, S):
    return np.unpackbits(g[key], axis=-1)[..., :S]


@pytest.fixture(scope="module")
def stroke_stats(g):
    """(band, differing, covered) of the restatement against RandomBrush's own masks, per set; computed once."""
    return {tag: R.compare_strokes(reference_cands(g, tag), unpack(g, f"{tag}.brush", S), S) for tag, S in SETS}


@pytest.mark.parametrize("tag,S", SETS[:2])
def test_geometry_is_the_references(g, tag, S):
    """Fed the fixture's draws, the restatement gives the reference's rectangles, vertex lists, widths, flips and the candidate its
    rejection loop ended on -- exactly."""
    ours, fell = R.geometry_batch(g[f"{tag}.u"], g[f"{tag}.z"], S)
    ref = R.pack(reference_cands(g, tag), S)
    assert fell == 0 and np.array_equal(ours["chosen"], g[f"{tag}.chosen"])
    assert g[f"{tag}.chosen"][0] == 3 and g[f"{tag}.chosen"][1] == 1          # the scripted empty candidates were consumed
    for k in ("rects", "verts", "nverts", "widths", "flips"):
        assert np.array_equal(ours[k], ref[k]), k
    n = g[f"{tag}.nverts"]
    assert n.max() == R.VERTS and n[n > 0].min() == 5 and (n > 0).sum(1).max() == R.STROKES
    w = g[f"{tag}.widths"][n > 0]
    assert w.min() >= 12 and w.max() <= 47 and g[f"{tag}.verts"].max() <= S and g[f"{tag}.verts"].min() == 0


@pytest.mark.parametrize("tag,S", SETS)
def test_rectangle_masks_are_bit_equal(g, tag, S):
    cands = reference_cands(g, tag)
    masks = unpack(g, f"{tag}.mask", S)
    ours = R.raster_batch(R.pack(cands, S), S)
    only = [b for b, c in enumerate(cands) if not c["strokes"]]
    assert len(only) >= (5 if tag.startswith("s") or tag == "hand64" else 0)
    for b in only:
        assert np.array_equal(ours[b], masks[b]), b
    if tag == "hand64":
        names = [str(n) for n in g["hand64.names"]]
        m = masks[names.index("rect_outside")]
        assert int((m == 0).sum()) == 4 * 5          # the rectangle beyond the corner covers nothing; its neighbour 4 x 5 pixels
        assert all(int((masks[names.index(n)] == 0).sum()) > 0 for n in names if n.startswith("rect_"))
    # with strokes, what differs from the reference's final mask differs in the strokes: never inside a rectangle
    for b, c in enumerate(cands):
        if c["strokes"] and c["raw_rects"]:
            p = R.pack([dict(c, strokes=[])], S)
            inside = R.raster(p["rects"][0], p["verts"][0], p["nverts"][0], p["widths"][0], p["flips"][0], S) == 0
            assert not (ours[b] != masks[b])[inside].any() and not masks[b][inside].any()


def test_strokes_match_pil_up_to_its_boundary_rounding(g, stroke_stats):
    differ = sum(v[1] for v in stroke_stats.values())
    covered = sum(v[2] for v in stroke_stats.values())
    for tag, (band, d, c) in stroke_stats.items():
        print(f"{tag}: band {band:.3f} px, {d} of {c} covered pixels differ ({100 * d / c:.2f} %)")
    print(f"fixture: {differ} of {covered} ({100 * differ / covered:.3f} %)")
    assert max(v[0] for v in stroke_stats.values()) <= BAND
    assert differ <= SHARE * covered
    assert differ > 0          # PIL is NOT matched bit for bit: an all-equal result would mean the comparison looks at nothing


def test_report_holds_what_the_fixture_gives(stroke_stats):
    rep = json.load(open(REPORT))
    assert rep["band_limit_px"] == BAND and rep["share_limit"] == SHARE
    for tag, (band, d, c) in stroke_stats.items():
        assert rep["sets"][tag]["differing_pixels"] == d and rep["sets"][tag]["pil_covered_pixels"] == c
        assert rep["sets"][tag]["band_px"] == pytest.approx(band, abs=1e-9)
    assert rep["fixture"]["band_px"] <= BAND and rep["fixture"]["share"] <= SHARE


def test_flip_cases_mirror_the_strokes_only(g):
    names = [str(n) for n in g["hand64.names"]]
    cands = reference_cands(g, "hand64")
    ours = R.raster_batch(R.pack(cands, 64), 64)
    base = cands[names.index("flip00")]
    strokes = 1 - R.brush_only(dict(base, flips=(0, 0)), 64)          # keep = 1
    p = R.pack([dict(base, strokes=[])], 64)
    rect = R.raster(p["rects"][0], p["verts"][0], p["nverts"][0], p["widths"][0], (0, 0), 64)
    for a in (0, 1):
        for b in (0, 1):
            s = np.flip(strokes, 0) if a else strokes
            s = np.flip(s, 1) if b else s
            assert np.array_equal(ours[names.index(f"flip{a}{b}")], s & rect), (a, b)
    assert len({ours[names.index(f"flip{a}{b}")].tobytes() for a in (0, 1) for b in (0, 1)}) == 4


def test_hole_ratio_statistics(g):
    """4096 restated masks from torch CPU draws at the recorded size: the mean hole ratio lies within 4 standard errors (the
    reference's recorded standard deviation / sqrt(4096)) of the mean the unpatched reference gave under numpy's generator.  At the
    recorded size, 64, the reference's redraw of all-hole candidates, which is not restated, lowers its mean by about one such error."""
    S, N = int(g["stat.size"]), int(g["stat.n"])
    gen = torch.Generator().manual_seed(22)
    u = torch.rand(N, R.CANDIDATES, R.NU, generator=gen).numpy()
    z = torch.randn(N, R.CANDIDATES, R.NZ, generator=gen).numpy()
    p, fell = R.geometry_batch(u, z, S)
    ratio = 1.0 - R.raster_batch(p, S).reshape(N, -1).mean(1)
    se = float(g["stat.std"]) / float(np.sqrt(N))
    print(f"hole ratio: restated {ratio.mean():.4f} +- {ratio.std(ddof=1):.4f}, reference {float(g['stat.mean']):.4f} +- "
          f"{float(g['stat.std']):.4f}, se {se:.4f}; first candidate empty {float((p['chosen'] > 0).mean()):.4f}, fell back {fell}")
    assert abs(float(ratio.mean()) - float(g["stat.mean"])) <= 4 * se
    assert fell == 0 and 0.005 <= float((p["chosen"] > 0).mean()) <= 0.03          # P(empty) = 1.55 % measured


def test_first_non_empty_candidate_is_kept():
    S = 64
    gen = torch.Generator().manual_seed(3)
    u, z = torch.rand(3, R.CANDIDATES, R.NU, generator=gen).numpy(), torch.randn(3, R.CANDIDATES, R.NZ, generator=gen).numpy()
    empty = [R.U_NRECT_SMALL, R.U_NRECT_BIG, R.U_NSTROKE]
    u[:, :, R.U_NSTROKE] = 0.6                      # every slab has strokes ...
    u[0, :2, empty] = 0.0                           # ... but sample 0's first two
    u[1, :, empty] = 0.0                            # ... and all of sample 1's
    u[2, 0, empty] = [0.9, 0.0, 0.0]                # sample 2's first: three rectangles, each of width or height 0
    u[2, 0, R.U_RECT:R.U_RECT + 12] = [0.0, 0.5, 0.5, 0.5, 0.5, 0.0, 0.5, 0.5, 0.0, 0.0, 0.5, 0.5]
    p, fell = R.geometry_batch(u, z, S)
    assert p["chosen"].tolist() == [2, 3, 1] and fell == 1
    masks = R.raster_batch(p, S)
    assert masks[1].all() and not masks[0].all() and not masks[2].all()          # the fallback's mask is all ones
    assert R.geometry(u[0], z[0], S)[1] == R.candidate(u[0, 2], z[0, 2], S)


def test_slot_table_is_defined_once_and_matches_the_header():
    from adm_amd.ddm import inpaint_data as T
    header = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    macros = {k: int(v) for k, v in re.findall(r"^#define ADM_INP_(\w+)\s+(\d+)\s*$", header, flags=re.M)}
    mine = {"CANDIDATES": T.CANDIDATES, "RECTS": T.RECTS, "STROKES": T.STROKES, "VERTS": T.VERTS, "SEGMENTS": T.SEGMENTS,
            "U_NRECT_SMALL": T.U_NRECT_SMALL, "U_RECT": T.U_RECT, "U_NRECT_BIG": T.U_NRECT_BIG, "U_NSTROKE": T.U_NSTROKE,
            "U_STROKE": T.U_STROKE, "STROKE_U": T.STROKE_U, "U_FLIP": T.U_FLIP, "NU": T.NU, "NZ": T.NZ}
    tile = {k: macros.pop(k) for k in ("TILE_H", "TILE_W")}
    assert macros == mine and tile["TILE_H"] * tile["TILE_W"] == 256
    # no slot is used twice, none is left over
    used = [T.U_NRECT_SMALL, T.U_NRECT_BIG, T.U_NSTROKE, T.U_FLIP, T.U_FLIP + 1] + list(range(T.U_RECT, T.U_RECT + 4 * T.RECTS))
    for s in range(T.STROKES):
        base = T.U_STROKE + s * T.STROKE_U
        used += [base + T.S_NUM_VERTEX, base + T.S_ANGLE_MIN, base + T.S_ANGLE_MAX, base + T.S_START, base + T.S_START + 1,
                 base + T.S_WIDTH, base + T.S_DISCARD, base + T.S_DISCARD + 1] + list(range(base + T.S_ANGLES, base + T.S_ANGLES + T.SEGMENTS))
    assert sorted(used) == list(range(T.NU)) and T.NZ == T.STROKES * T.SEGMENTS
    # the restatement and the stream import the table, they do not restate it
    for path in (os.path.join(HERE, "inpaint_ref.py"), os.path.join(ROOT, "tools", "make_golden_inpaint.py")):
        assert not re.search(r"^\s*(NU|NZ|U_FLIP|U_STROKE|STROKE_U)\s*=\s*\d", open(path).read(), flags=re.M), path
    assert R.NU is T.NU


def test_entry_points_are_declared_and_bound():
    from adm_amd import hip
    header = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    for name, n in (("adm_inpaint_masks", 12), ("adm_inpaint_batch", 18), ("adm_inpaint_compose", 8)):
        m = re.search(rf"^int\s+{name}\s*\(([^;]*?)\)\s*;", header, flags=re.M | re.S)
        assert m and m.group(1).count(",") + 1 == n == len(hip._SIGS[name]), name
    assert "inpaint_data.hip" in open(os.path.join(ROOT, "adm_amd", "csrc", "Makefile")).read()


def test_stream_error_paths(tmp_path):
    from adm_amd.ddm.inpaint_data import HOLDOUT, InpaintBatchStream, load_inpaint_folder
    cpu = torch.device("cpu")
    np.save(tmp_path / "wide.npy", np.zeros((2, 32, 40, 3), np.uint8))
    np.save(tmp_path / "ok.npy", np.zeros((2, 32, 32, 3), np.uint8))
    with pytest.raises(ValueError, match="square and equal to image_size 32"):
        InpaintBatchStream({"npy": str(tmp_path / "wide.npy")}, 2, (32, 32), cpu, 1)
    with pytest.raises(ValueError, match="square and equal to image_size 64"):
        InpaintBatchStream({"npy": str(tmp_path / "ok.npy")}, 2, (64, 64), cpu, 1)
    with pytest.raises(ValueError, match="square image_size"):
        InpaintBatchStream({"npy": str(tmp_path / "wide.npy")}, 2, (32, 40), cpu, 1)
    with pytest.raises(NotImplementedError, match="hole_range"):
        InpaintBatchStream({"npy": str(tmp_path / "ok.npy"), "hole_range": [0.2, 0.8]}, 2, (32, 32), cpu, 1)
    with pytest.raises(NotImplementedError, match="class_name"):
        InpaintBatchStream({"class_name": "ddm.data.EdgeDataset"}, 2, (32, 32), cpu, 1)
    with pytest.raises(ValueError, match="img_folder"):
        InpaintBatchStream({"class_name": "ddm.data.InpaintDataset"}, 2, (32, 32), cpu, 1)
    s = InpaintBatchStream({"npy": str(tmp_path / "ok.npy"), "hole_range": [0, 1]}, 2, (32, 32), cpu, 1)
    assert s.pool.n == 2 and int(s.fallbacks) == 0
    with pytest.raises(RuntimeError, match="needs a GPU tensor"):          # no CPU fallback
        s.next_batch()
    # the folder: *.jpg only, not recursive, sorted; the last HOLDOUT files are the test split
    from PIL import Image
    folder = tmp_path / "faces"
    (folder / "sub").mkdir(parents=True)
    for name in ("b.jpg", "a.jpg", "c.png", "sub/d.jpg"):
        Image.fromarray(np.full((32, 32, 3), 7, np.uint8)).save(folder / name)
    with pytest.raises(ValueError, match="2 jpg files, so split 'train' is empty"):
        InpaintBatchStream({"class_name": "ddm.data.InpaintDataset", "img_folder": str(folder)}, 2, (32, 32), cpu, 1)
    images, names = load_inpaint_folder(str(folder), "test")
    assert names == ["a.jpg", "b.jpg"] and images[0].shape == (32, 32, 3) and HOLDOUT == 2000
    s = InpaintBatchStream({"class_name": "ddm.data.InpaintDataset", "img_folder": str(folder), "split": "test"}, 2, (32, 32), cpu, 1)
    assert s.pool.n == 2
    with pytest.raises(ValueError, match="square and equal"):
        InpaintBatchStream({"class_name": "ddm.data.InpaintDataset", "img_folder": str(folder), "split": "test"}, 2, (16, 16), cpu, 1)
