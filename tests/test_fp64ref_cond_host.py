"""CPU: the net of tests/test_hip_cond_accuracy.py tested without a GPU.

(a) every reference of the SR denoiser's family in tests/fp64ref.py against an independently written fp64 formulation (F.batch_norm,
    F.interpolate, F.fold, softmax / einsum compositions, autograd) on every case of tests/cond_cases.py, to 1e-12 of the
    output's own maximum (of max mag where the output is analytically zero);
(b) teeth: fp32 implementations with one deliberate defect each miss the bar the GPU test applies to the case, while correct fp32
    torch passes it.  Two of them can only show as NaN / inf: "lse without the running max" is the same function as the correct
    softmax wherever exp() does not overflow (on the dominant row, logits of ~ 12, it is exact and passes), so what the x6 rows show
    is that an overflow is noticed; "eps dropped" misses the bar by finite amounts on the eps rows and by 0 x inf on the const rows;
(c) the fallback bar is used exactly where it is needed: fp32 torch is above BAR_A / 4 on the cases of cond_cases.FALLBACK and at or
    below BAR_A / 4 on every other case;
(d) the table as a whole holds the geometries it was written for.
"""
import functools

import pytest
import torch

import cond_cases as cc
import fp64ref
from test_hip_accuracy import BAR_A

ALL = [(op, c) for op in cc.OPS for c in cc.CASES[op]]
ALL_IDS = [f"{op}-{c[0]}" for op, c in ALL]


@functools.lru_cache(maxsize=None)
def _e32(op, name):
    """e_max of plain fp32 torch against the fp64 reference, per output."""
    case = cc.by_id(op, name)
    data = cc.make(op, case)
    ref = cc.reference(op, case, data)
    got = cc.torch32(op, case, data)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    return {n: fp64ref.errors(got[n], *ref[n])[0] for n in ref}


def _limit(op, case, n):
    """The bar of the GPU test for output n of a case."""
    return max(BAR_A, 2.0 * _e32(op, case[0])[n]) if cc.is_fallback(op, case) else BAR_A


@pytest.mark.parametrize("op,case", ALL, ids=ALL_IDS)
def test_reference_matches_independent_fp64(op, case):
    """The torch composition of cond_cases (torch's own operators, autograd's gradients) run in fp64 agrees with the reference
    written from the definition to 1e-12 relative to the output's own maximum; every mag bounds |ref|.  An output that is zero
    analytically (mha's dq with all keys equal, dq / dk of a single key, SpatialAtt's dqk on one pixel: max |t| below 1e-9 of
    max mag) has no scale of its own: there the two must agree to 1e-12 of max mag, and exactly where mag is zero too."""
    data = cc.make(op, case)
    ref = cc.reference(op, case, data)
    want = cc.torch32(op, case, {k: v.double() for k, v in data.items()})
    assert set(ref) == set(want)
    for n, (r, mag) in ref.items():
        t = want[n]
        assert r.shape == t.shape and mag.shape == t.shape, (n, r.shape, mag.shape, t.shape)
        assert r.dtype == torch.float64 and t.dtype == torch.float64
        scale, mscale = float(t.abs().max()), float(mag.max())
        if scale < 1e-9 * mscale or scale == 0.0:
            scale = mscale
        assert float((r - t).abs().max()) <= 1e-12 * scale, (n, float((r - t).abs().max()), scale)
        assert bool((mag >= r.abs() * (1 - 1e-9)).all()), n
    if op != "fourier" and op != "col2im":
        fwd = cc.reference(op, case, data, backward=False)
        assert set(fwd) < set(ref) and all(torch.equal(fwd[n][0], ref[n][0]) for n in fwd)


@pytest.mark.parametrize("op,case", ALL, ids=ALL_IDS)
def test_fallback_bar_is_used_exactly_where_fp32_needs_it(op, case):
    e = _e32(op, case[0])
    print(f"{op} {case[0]}: fp32 torch " + " ".join(f"{n} {v:.2e}" for n, v in e.items()))
    if cc.is_fallback(op, case):
        assert max(e.values()) > BAR_A / 4, "marked for the fallback bar, but plain fp32 does not need it"
    else:
        assert max(e.values()) <= BAR_A / 4, "plain fp32 needs the fallback bar here: mark the case (and say why) or change its data"


def test_fallback_names_exist():
    for op, names in cc.FALLBACK.items():
        assert set(names) <= set(cc.ids(op)), (op, names)


# ------------------------------------------------------------------------------------------------ (b) the bar has teeth
_TRAIN_BN = ["M3-C1024-train-plain", "M257-C384-train-offset", "M513-C4-train-eps", "M1025-C12-train-const", "M8200-C512-train-plain"]
TEETH = [
    # op, defect, the cases on which it must be seen, the output that must miss the bar (None: any)
    ("ws", "eps dropped", ["K63-eps", "K288-const", "K1152-eps"], None),
    ("ws", "eps 1e-3", ["K63-eps", "K288-const", "K1152-eps"], None),
    ("ws", "unbiased variance", cc.ids("ws"), None),
    ("ln", "eps dropped", ["M3-C12-eps", "M257-C384-eps", "M257-C1024-const", "M524800-C4-eps"], None),
    ("ln", "eps 1e-3", ["M3-C12-eps", "M257-C384-eps", "M257-C1024-const", "M524800-C4-eps"], None),
    ("ln", "unbiased variance", [n for n in cc.ids("ln") if n != "M1-C4-const"], None),      # (its only row has variance 0 either way)
    ("bn", "eps dropped", ["M513-C4-train-eps", "M1025-C12-train-const", "M1025-C128-eval-eps"], None),
    # (at M = 524 800 the two variances differ by 2e-6: out of any fp32 bar's reach, and of no consequence)
    ("bn", "unbiased variance", _TRAIN_BN, "y"),
    # (momentum / M = 3.7e-6 of the variance at M = 8200: the running variance shows the divisor only at the smaller M)
    ("bn", "biased running variance", _TRAIN_BN[:-1], "running_var"),
    ("bilinear", "wrong align_corners", [n for n in cc.ids("bilinear") if not n.startswith(("same", "1x1"))], None),
    ("la", "missing 1/N", [n for n in cc.ids("la") if n != "N1"], None),
    ("la", "key softmax over the wrong axis", cc.ids("la"), None),
    ("mha", "scale applied twice", ["packed-L256-D32", "packed-L65-D32-x6"], None),
    ("mha", "lse without the running max", [n for n in cc.ids("mha") if n.endswith("x6")], None),
    ("spatt", "softsign derivative without the square", cc.ids("spatt"), "datt"),
]


def test_every_defect_has_a_row():
    assert {(op, d) for op, d, _, _ in TEETH} == {(op, d) for op, ds in cc.DEFECTS.items() for d in ds}


@pytest.mark.parametrize("op,defect,names,output", TEETH, ids=[f"{t[0]}-{t[1].replace(' ', '-').replace('/', '-')}" for t in TEETH])
def test_bar_rejects_defect(op, defect, names, output):
    """A defective fp32 implementation misses the bar of the GPU test on every listed case (a NaN misses it too); correct fp32 torch
    passes the same bar on the same data."""
    for name in names:
        case = cc.by_id(op, name)
        data = cc.make(op, case)
        ref = cc.reference(op, case, data)
        bad = cc.torch32(op, case, data, defect=defect)
        e = {n: fp64ref.errors(bad[n], *ref[n])[0] for n in ref}
        missed = [n for n in ref if not e[n] <= _limit(op, case, n)]
        print(f"{op} {name} [{defect}]: " + " ".join(f"{n} {v:.2e}" for n, v in e.items()) + f"; misses the bar on {missed}")
        assert missed, (name, e)
        if output is not None:
            assert output in missed, (name, output, e)
        for n, v in _e32(op, name).items():
            assert v <= _limit(op, case, n), (name, n, v)


# ------------------------------------------------------------------------------------------------ (d) the table's geometry
def test_table_covers_the_unexercised_paths():
    ws, ln, bn = cc.CASES["ws"], cc.CASES["ln"], cc.CASES["bn"]
    norm_C = {c[2] for c in ln} | {c[2] for c in bn}
    assert {4, 12, 384, 1024} <= norm_C
    K = {c[2] * c[3] * c[3] for c in ws}
    assert 63 in K and any(k > 256 and k % 256 for k in K)
    assert {1, 3, 257} <= {c[1] for c in ln} and {513, 1025} <= {c[1] for c in bn}
    assert any(c[1] > 524288 and c[2] == 4 for c in ln) and any(c[1] > 524288 and c[2] == 4 and c[4] for c in bn)
    for op, kinds in (("ws", {c[4] for c in ws}), ("ln", {c[3] for c in ln}), ("bn", {c[3] for c in bn})):
        assert {"eps", "const", "offset"} <= kinds, op
    assert {True, False} == {c[4] for c in bn}
    quads = 1048576                                          # 4096 workgroups x 256 threads: above it co_grid's kernels loop
    assert any(c[1] * c[2] // 4 > quads and c[4] for c in bn)
    assert any(c[1] * c[4] * c[5] * c[6] // 4 > quads for c in cc.CASES["bilinear"])
    assert any(torch.Size(c[1]).numel() // 4 > quads for c in cc.CASES["act"])
    assert any(c[1] * c[2] * c[3] * c[4] // 4 > quads for c in cc.CASES["col2im"])
    bl = cc.CASES["bilinear"]
    assert {True, False} == {c[7] for c in bl} and any(c[2] == 128 for c in bl) and any(c[2] == c[3] == 1 for c in bl)
    assert any((c[2], c[3]) == (c[4], c[5]) for c in bl) and any(c[4] < c[2] for c in bl) and any(c[4] > c[2] for c in bl)
    assert {3} <= {c[8][0] for c in bl if c[8]} and any(c[8][0] % 4 == 0 for c in bl if c[8])
    mha = cc.CASES["mha"]
    assert {1, 63, 64, 65, 130} <= {c[2] for c in mha} and {1, 63, 64, 65, 130, 1024} <= {c[3] for c in mha}
    assert {16, 32, 64} <= {c[5] for c in mha} and {"x6", "equal", "dominant"} <= {c[7] for c in mha} and any(c[8] for c in mha)
    assert any(c[2] > 64 and c[2] % 64 for c in mha)
    la = cc.CASES["la"]
    assert {1, 63, 65, 1025, 16384} <= {c[2] for c in la} and any(c[3] == "spread" and c[2] > 1024 for c in la)
    sp = cc.CASES["spatt"]
    assert {1, 257, 2560} <= {c[2] * c[3] for c in sp}
    assert any(c[5][0] > 0 for c in sp) and any(c[5][0] < 0 for c in sp) and any(c[5][0] == 0 for c in sp)
    assert all(c[1] <= 2 for op in cc.OPS for c in cc.CASES[op] if op in ("bilinear", "mha", "la", "spatt", "col2im"))
