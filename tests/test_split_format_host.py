"""CPU: the one statement of the split number formats (adm_amd/csrc/split_format.h) against numpy.

tests/host/split_format_check.cpp is compiled host-only with the Makefile's compiler and run on the CPU; what it prints is compared
with restatements of the scale rule, the two splits, the overflow predicate and the two weight-image layouts written here in numpy.
The GPU tests that compare a pack kernel with a split kernel compare two users of that header; this is the independent check."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adm_amd", "csrc")
f32, f16 = np.float32, np.float16


def _hipcc():
    default = re.search(r"^HIPCC\s*\?=\s*(\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    return os.environ.get("HIPCC", default)      # `?=`: the environment wins, as it does for make


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """run(mode, *args, data=None) -> the program's stdout bytes; `data` (float32) goes in through a file"""
    tmp = tmp_path_factory.mktemp("split_format")
    exe = str(tmp / "split_format_check")
    r = subprocess.run([_hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17", os.path.join(ROOT, "tests", "host", "split_format_check.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(mode, *args, data=None):
        argv = [exe, mode]
        if data is not None:
            path = str(tmp / (mode + ".f32"))
            np.asarray(data, f32).tofile(path)
            argv.append(path)
        r = subprocess.run(argv + [str(a) for a in args], capture_output=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    return run


def _values():
    """4096 seeded float32 bit patterns + the edge cases (the overflow threshold and its neighbour below, +-0, the smallest and the largest normal numbers of both signs, two
    denormals).  The splits are statements about NUMBERS (a0 + a1 + a2 == a has no meaning for inf - inf), so a drawn pattern with the
    exponent field 255 (inf / NaN, 1 in 256) gets the field's top bit cleared; exponent 0 (denormals and zeros) stays."""
    bits = np.random.default_rng(20240607).integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32)
    bits = np.where((bits >> 23) & 0xFF == 0xFF, bits & ~np.uint32(0x40000000), bits).astype(np.uint32)
    edge = np.array([0x00000000, 0x80000000, 0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000123, 0x807FFFFF], np.uint32)
    lim = f32(65000)                                 # the overflow threshold itself, reached at both scales of the two-term test
    at = np.array([lim, -lim, np.nextafter(lim, f32(0)), lim / f32(2048), np.nextafter(lim / f32(2048), f32(0))], f32).view(np.uint32)
    v = np.concatenate([bits, at, edge]).view(f32)
    assert np.isfinite(v).all()
    return v


def test_scale_rule(check):
    """s = 2^(e - 1) with 16000 / bound = m 2^e, m in [0.5, 1): 16000 / bound < 2 s <= 32000 / bound ... in float32, as the kernels
    compute it; 1 for a bound that is no positive number below 3e38"""
    b0 = f32(15.625)                                 # s * b = 16000 exactly
    bounds = np.array([0.0, -1.0, np.nan, np.inf, 3e38, 1e-30, 1e-6, 15.0, np.nextafter(b0, f32(0)), b0, np.nextafter(b0, f32(100)),
                       1e4, 65504.0], f32)
    got = np.frombuffer(check("scale", data=bounds), f32)
    assert got.shape == bounds.shape
    with np.errstate(all="ignore"):
        live = (bounds > 0) & (bounds < f32(3e38))
        m, e = np.frexp(f32(16000) / np.where(live, bounds, f32(1)))
    want = np.where(live, np.ldexp(f32(1), e - 1), f32(1)).astype(f32)
    print(np.stack([bounds, got, want], 1))
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert (np.frexp(got)[0] == 0.5).all()           # a power of two
    assert not live[:5].any() and live[5:].all()
    assert got[9] * b0 == 16000 and got[8] == got[9] and got[10] == got[9] / 2       # the exponent changes right above 15.625


def test_three_term_split(check):
    """a0 + a1 + a2 == a EXACTLY, every term with its low 16 bits clear -- wherever f32 can hold the terms: a = m 2^E leaves
    a - a0 - a1 = k 2^(E - 23), k < 2^8, which has <= 8 significant bits as a NORMAL number, i.e. for E >= -103 (exponent field >= 24),
    and for a bf16 number (0 is one).  Below that a remainder is a denormal, whose top 16 bits are its multiples of 2^-133: what is lost is < 2^-133.  Uniform
    bit patterns put 9 % of the inputs there, so both statements are asserted, each on its inputs; the terms themselves are compared
    bit for bit with the restated arithmetic on all of them."""
    v = _values()
    t = np.frombuffer(check("split3", data=v), np.uint16).reshape(3, -1)
    assert t.shape[1] == v.size
    bits = v.view(np.uint32)
    exact = ((bits >> 23) & 0xFF >= 24) | (bits & 0xFFFF == 0)          # (or a is a bf16 number itself: +-0, the smallest normals)
    print("inputs:", v.size, "with exact terms:", int(exact.sum()))
    assert exact[-8:-2].all() and not exact[-2:].any() and (~exact).sum() > 100
    # a stored term IS 16 bits (the top half of an f32 term), so the stored terms sum to a only if the low halves were clear
    terms = (t.astype(np.uint32) << 16).view(f32).astype(np.float64)     # 3 x 8 mantissa bits within 24: exact in float64
    lost = np.abs(v.astype(np.float64) - (terms[0] + terms[1] + terms[2]))
    assert (lost[exact] == 0).all()
    assert (lost < 2.0 ** -133).all()
    assert (t[0] == (bits >> 16)).all()                                  # a0 = the top 16 bits of a
    r1 = v - (bits & 0xFFFF0000).view(f32)
    assert (t[1] == (r1.view(np.uint32) >> 16)).all()                    # a1 = the top 16 bits of a - a0
    r2 = r1 - (r1.view(np.uint32) & 0xFFFF0000).view(f32)
    assert (t[2] == (r2.view(np.uint32) >> 16)).all()                    # a2 = a - a0 - a1 ...
    assert (r2.view(np.uint32)[exact] & 0xFFFF == 0).all()               # ... whole


@pytest.mark.parametrize("s", [1.0, 2048.0])
def test_two_term_split_and_overflow(check, s):
    v = _values()
    out = check("split2", s, data=v)
    n = v.size
    t = np.frombuffer(out[:4 * n], np.uint16).reshape(2, n)
    bad = np.frombuffer(out[4 * n:], np.uint8)
    assert bad.size == n
    with np.errstate(all="ignore"):
        x = v * f32(s)
        h0 = x.astype(f16)
        h1 = (x - h0.astype(f32)).astype(f16)        # (inf - inf = NaN where the scaled value overflowed: same operation on both sides)
    print("overflowing:", int(bad.sum()), "of", n)
    assert (t[0] == h0.view(np.uint16)).all()
    assert (t[1] == h1.view(np.uint16)).all()
    assert (bad.astype(bool) == ~(np.abs(x) < f32(65000))).all()
    assert bad.any() and not bad.all()


@pytest.mark.parametrize("terms", [3, 2])
@pytest.mark.parametrize("rows,cols", [(32, 16), (96, 64)])
def test_image_layouts(check, rows, cols, terms):
    o = np.frombuffer(check("layout", rows, cols, terms), np.int64)
    nw, nr = 16 * terms * rows * cols, terms * rows * cols
    assert o.size == nw + nr
    # [ey][cols/16][ex][term][rows][16], asked for in the order [ey][ex][term][n][c]
    w = np.arange(nw).reshape(4, cols // 16, 4, terms, rows, 16).transpose(0, 2, 3, 4, 1, 5).reshape(-1)
    assert (o[:nw] == w).all()
    assert (np.sort(o[:nw]) == np.arange(nw)).all()
    # [cols/16][term][rows][16], asked for in the order [term][n][c]
    r = np.arange(nr).reshape(cols // 16, terms, rows, 16).transpose(1, 2, 0, 3).reshape(-1)
    assert (o[nw:] == r).all()
    assert (np.sort(o[nw:]) == np.arange(nr)).all()
