"""CPU-only: the split count of the 3x3 weight gradient (conv_wgrad_x6.hip) as host queries.

adm_conv_wgrad_x6_h3_plan is the count the fp16-format launch takes in the atomic mode.  Where its 128-cout workgroups qualify it is the
minimum of a time model -- rounds of 256 workgroups x (stages of a split + the epilogue in stages) -- wherever that beats the fill rule
by more than 5 %, and the fill rule's count everywhere else.  adm_conv_wgrad_x6_plan is the deterministic mode's count (the caller
sizes its workspace by it): the fill rule, unchanged.  The model and the fill rule are restated here."""
import ast
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPI_ATOMIC, EPI_STORE = 15, 5      # the epilogue of a split in stages: float atomics (more than one split), plain stores (one)


@pytest.fixture(scope="module")
def lib():
    from adm_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip.lib()


def cdiv(a, b):
    return -(-a // b)


def real_splits(Pp, s):
    chunk = cdiv(cdiv(Pp, s), 16) * 16
    return cdiv(Pp, chunk)


def fill_rule(tiles, Pp):
    maxs = min(cdiv(Pp, 96), 64)
    best, splits = -1.0, 1
    for s in range(1, maxs + 1):
        wgs = tiles * s
        fill = wgs / (cdiv(wgs, 256) * 256) - 0.002 * s
        if fill > best + 1e-9:
            best, splits = fill, s
    return real_splits(Pp, splits)


def model_time(tiles, Pp, s):
    return cdiv(tiles * s, 256) * (cdiv(cdiv(Pp, s), 16) + (EPI_ATOMIC if s > 1 else EPI_STORE))


def production_shapes():
    """(H, W, Cin, Cout) of every 3x3 weight gradient on the fp16 format that a shipped config launches: the census table of
    tests/test_hip_accuracy.py, read as text (importing that module would collect its GPU tests here)."""
    src = open(os.path.join(ROOT, "tests", "test_hip_accuracy.py")).read()
    a = src.index("PRODUCTION_LAUNCHES = {")
    table = ast.literal_eval(src[a + len("PRODUCTION_LAUNCHES = "):src.index("\n}\n", a) + 2])
    out = set()
    for keys in table.values():
        for name, ints, _ in keys:
            if name == "adm_conv_wgrad_x6_h3":
                out.add((ints[1], ints[2], ints[3], ints[5]))
    assert len(out) >= 30
    return sorted(out)


@pytest.mark.parametrize("B", [1, 16, 128])
def test_time_plan_is_admissible_and_never_modelled_slower_than_the_fill_rule(lib, B):
    changed = 0
    for H, W, cin, cout in production_shapes():
        Pp = B * H * W // 4
        s = lib.adm_conv_wgrad_x6_h3_plan(B, H, W, cin, cout)
        maxs = min(cdiv(Pp, 96), 64)
        assert 1 <= s <= max(maxs, 1), (B, H, cin, cout, s)      # maxs: the floor of 6 stages (96 tiles) per split, and the cap
        assert real_splits(Pp, s) == s, "no empty split"
        cb = 2 if cout > 64 else 1
        tiles = cdiv(cout, 64 * cb) * cdiv(cin, 64) * 4
        f = fill_rule(tiles, Pp)
        if cb == 1:
            assert s == f, "64-cout workgroups keep the fill rule"
            continue
        assert model_time(tiles, Pp, s) <= model_time(tiles, Pp, f)
        if s != f:          # overruled only where the model is more than 5 % ahead, and then with its minimum
            changed += 1
            assert model_time(tiles, Pp, s) * 21 < model_time(tiles, Pp, f) * 20
            assert model_time(tiles, Pp, s) == min(model_time(tiles, Pp, k) for k in range(1, maxs + 1) if real_splits(Pp, k) == k)
    if B == 128:
        assert changed >= 4


# (B, H, Cin, Cout) -> splits: what the forced-split sweep of tools/bench_wgrad_x6.cpp measured fastest (first four: the plan moved),
# or within 3 % of the fastest (the rest: the plan stayed)
SWEPT = {(128, 8, 384, 384): 3, (128, 8, 768, 384): 3, (128, 4, 768, 384): 1, (128, 16, 192, 192): 10,
         (128, 4, 384, 384): 3, (128, 16, 384, 384): 7, (128, 16, 768, 384): 7, (128, 16, 192, 384): 7, (128, 16, 576, 384): 7,
         (128, 32, 192, 192): 21, (128, 32, 384, 192): 16, (128, 32, 576, 192): 7, (128, 32, 384, 384): 7}


def test_plan_on_the_swept_shapes(lib):
    got = {k: lib.adm_conv_wgrad_x6_h3_plan(k[0], k[1], k[1], k[2], k[3]) for k in SWEPT}
    assert got == SWEPT


# (B, H, Cin, Cout, splits) of adm_conv_wgrad_x6_plan, recorded before the time model: the deterministic mode's plan has not moved
DET_PLAN = ((128, 4, 384, 384, 5), (128, 4, 768, 384, 6), (128, 8, 384, 384, 7), (128, 8, 768, 384, 8), (128, 8, 192, 32, 19),
            (128, 16, 192, 192, 7), (128, 16, 768, 384, 8), (128, 16, 192, 32, 21), (128, 32, 32, 32, 64), (128, 32, 128, 128, 16),
            (128, 32, 576, 192, 7), (16, 32, 32, 32, 43), (16, 32, 192, 32, 20), (16, 16, 128, 128, 11), (16, 8, 576, 192, 2),
            (16, 64, 1024, 512, 1), (1, 32, 384, 384, 3), (1, 64, 64, 64, 11), (1, 16, 768, 384, 1), (128, 4, 1024, 512, 1))


def test_deterministic_plan_is_unchanged(lib):
    for B, H, cin, cout, want in DET_PLAN:
        assert lib.adm_conv_wgrad_x6_plan(B, H, H, cin, cout) == want, (B, H, cin, cout)


def test_query_rejects_what_the_launcher_rejects(lib):
    assert lib.adm_conv_wgrad_x6_h3_plan(2, 6, 8, 64, 64) < 0       # H not a power of two
    assert lib.adm_conv_wgrad_x6_h3_plan(2, 8, 8, 48, 64) < 0       # Cin not a multiple of 32
    assert lib.adm_conv_wgrad_x6_h3_plan(0, 8, 8, 64, 64) < 0
