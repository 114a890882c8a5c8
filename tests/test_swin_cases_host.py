"""CPU-only: the tables of the Swin encoder kernel sweep (tests/swin_cases.py) -- the forms they reach, both sides of the backward
grids' caps, and the comments of csrc/swin.hip / include/adm_hip.h against the form queries.

adm_ln_form and adm_patch_embed_form are the functions through which ln_launch / ln_bwd_launch and PE_DISPATCH / pe_token_groups choose
their instantiation, so what they answer is what runs.
"""
import ctypes
import os
import re

import swin_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
SOURCE = open(os.path.join(ROOT, "adm_amd", "csrc", "swin.hip")).read()


def test_queries_are_declared_exported_and_used():
    from adm_amd import hip
    assert re.search(r"^int\s+adm_ln_form\s*\(int C, int\* out\);", HEADER, flags=re.M)
    assert re.search(r"^int\s+adm_patch_embed_form\s*\(int E, int\* out\);", HEADER, flags=re.M)
    for name in ("adm_ln_form", "adm_patch_embed_form"):
        assert name in hip.EXPORTS and name in hip.NO_STREAM
    lib, out = hip.lib(), (ctypes.c_int * 3)()
    assert lib.adm_ln_form(64, None) == -22 and lib.adm_patch_embed_form(64, None) == -22
    assert [lib.adm_ln_form(C, out) for C in (0, -4, 28, 34, 2052, 4096)] == [-22] * 6
    assert [lib.adm_patch_embed_form(E, out) for E in (0, -32, 16, 48, 100, 544)] == [-22] * 6
    # the rule exists once: both launch helpers and the stem dispatch call the form functions, nothing else derives a form
    assert SOURCE.count("ln_form(C, form)") == 3 and SOURCE.count("(C / 4 + 63) / 64") == 0          # the export and the two launches
    assert "pe_form((E), form_)" in SOURCE and SOURCE.count("pe_form(E, form)") == 2                 # the export and pe_token_groups
    assert not re.search(r"\(E\) <= \d+\) PE_GO", SOURCE)


def test_ln_tables_reach_every_form_whole_and_partial():
    every = {f"{m}:NQ{nq}:{w}" for m in ("plain", "merge") for nq in (1, 2, 4, 8) for w in ("whole", "partial")}
    answerable = {sc.ln_label(m, C) for m in (False, True) for C in range(32, 2049, 4)}
    assert answerable == every
    assert sc.ln_forms_reached() == every
    # the paths the issue names
    assert sc.ln_form(768) == (4, 64) and sc.ln_label(False, 768) == "plain:NQ4:partial"          # an empty last trip
    assert sc.ln_form(260) == (2, 1) and sc.ln_form(36) == (1, 9) and sc.ln_form(2044) == (8, 63)
    assert [sc.ln_form(C)[0] for C in (32, 256, 260, 512, 516, 1024, 1028, 2048)] == [1, 1, 2, 2, 4, 4, 8, 8]
    assert sorted({C for _, C in sc.LN_CASES}) == [32, 36, 96, 256, 260, 384, 512, 640, 768, 1024, 1536, 2044, 2048]
    for C in sc.LN_C:
        assert {M for M, c in sc.LN_CASES if c == C} >= {1, 3, 37}
    # merged: a Cin that is no power of two in every NQ (quad = c / Cin is a real division)
    pow2 = lambda n: n & (n - 1) == 0
    assert {sc.ln_form(4 * c[3])[0] for c in sc.MERGE_CASES if not pow2(c[3])} == {1, 2, 4, 8}
    assert {c[3] for c in sc.MERGE_CASES} >= {8, 24, 96, 128, 192, 256, 384, 512}
    for Cin in (24, 128):
        assert {(c[1], c[2]) for c in sc.MERGE_CASES if c[3] == Cin} >= {(1, 1), (1, 5), (5, 1), (3, 3), (4, 6), (9, 11)}
    # all eight row classes at M = 37, the constant row once
    cls = sc.row_classes(37)
    assert set(cls) == set(sc.LN_CLASSES) and cls["const"].tolist() == [7] and sum(len(v) for v in cls.values()) == 37


def test_stem_table_reaches_every_lane_layout():
    answerable = {sc.pe_label(E) for E in range(32, 513, 32)}
    assert answerable == {"G8Q1:exact", "G16Q1:exact", "G32Q1:exact", "G32Q1:past", "G64Q1:exact", "G64Q1:past", "G64Q2:exact", "G64Q2:past"}
    assert sc.pe_forms_reached() == answerable
    assert {sc.pe_form(E)[:2] for E in sc.STEM_E} == {(8, 1), (16, 1), (32, 1), (64, 1), (64, 2)}
    for E in sc.STEM_E:
        small = {(c.geom, c.content) for c in sc.STEM_CASES if c.E == E}
        assert small >= {(g, k) for g in sc.STEM_SMALL for k in sc.STEM_CONTENTS}, E
    assert any(c.geom[2] % 4 for c in sc.STEM_CASES) and any(sc.pe_tokens(c.geom) == 1 for c in sc.STEM_CASES)


def test_tables_reach_both_sides_of_both_block_caps():
    ln = {(M, C): sc.ln_bwd_blocks(M, C) for M, C in sc.LN_CASES}
    mg = {c: sc.ln_bwd_blocks(sc.merge_rows(c), 4 * c[3]) for c in sc.MERGE_CASES}
    for blocks in (ln, mg):
        assert min(blocks.values()) < sc.LN_BWD_MAXBLOCKS and max(blocks.values()) == sc.LN_BWD_MAXBLOCKS
    # capped means: more rows than 4 per wave of 256 workgroups, so a wave walks more than four rows
    assert all((b == sc.LN_BWD_MAXBLOCKS) == (M > 4 * sc.LN_ROWS * (sc.LN_BWD_MAXBLOCKS - 1)) for (M, _), b in ln.items())
    assert {k for k, b in ln.items() if b == 256} == {(4099, 32), (4099, 260)} and ln[(37, 32)] == 3 and ln[(1, 32)] == 1
    assert {k for k, b in mg.items() if b == 256} == {(2, 91, 91, 8)} and sc.merge_rows((2, 91, 91, 8)) == 4232
    pe = {(c.geom, c.E): sc.pe_bwd_blocks(c.geom, c.E) for c in sc.STEM_CASES}
    assert min(pe.values()) == 1 and max(pe.values()) == sc.PE_BWD_MAXBLOCKS
    capped = {k for k, b in pe.items() if b == sc.PE_BWD_MAXBLOCKS}
    assert capped == set(sc.STEM_CAPPED)
    assert [sc.pe_token_groups(g, E) for g, E in sc.STEM_CAPPED] == [4160, 4160, 4141] and sc.pe_tokens((1, 728, 728)) == 33124
    for (g, E), b in pe.items():
        want = -(-sc.pe_token_groups(g, E) // (4 * sc.PE_WAVES))
        assert b == min(max(want, 1), sc.PE_BWD_MAXBLOCKS), (g, E)
    # the attention table: a workgroup boundary crossed with every wave busy, and a last workgroup with an idle wave
    units = {sc.attn_units(g) for g in sc.ATTN_GEOM}
    assert any(u > 4 and u % 4 == 0 for u in units) and any(u % 4 == 3 for u in units) and 1 in units
    assert any(not sc.attn_padded(g) for g in sc.ATTN_GEOM) and any(g[4][0] != g[4][1] for g in sc.ATTN_GEOM)


def test_comments_say_what_the_queries_answer():
    """Supported C and E, and the dispatch line above PE_DISPATCH, in csrc/swin.hip and include/adm_hip.h."""
    doc = lambda name: re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+%s\s*\(" % name, HEADER, flags=re.S).group(1)
    m = re.search(r"(\d+) <= C <= (\d+), C % (\d+) == 0", doc("adm_ln_affine_fwd"))
    s = re.search(r"Supported C: (\d+) <= C <= (\d+), C % (\d+) == 0", SOURCE)
    rows = re.search(r"LayerNorm over rows of up to (\d+) floats", SOURCE)
    assert m and s and rows and m.groups() == s.groups() and rows.group(1) == m.group(2)
    lo, hi, step = (int(v) for v in m.groups())
    for C in range(1, 2200):
        assert (sc.ln_form(C) is not None) == (lo <= C <= hi and C % step == 0), C
    mm = re.search(r"C % 4 == 0, (\d+) <= C <= (\d+)\.", doc("adm_swin_merge_ln_fwd"))
    assert mm and [4 * int(v) for v in mm.groups()] == [lo, hi]
    # "the smallest of 1, 2, 4, 8 that covers the row"
    assert "the smallest of 1, 2, 4, 8 that covers the row" in SOURCE
    for C in range(lo, hi + 1, step):
        nq, last = sc.ln_form(C)
        assert nq == min(n for n in (1, 2, 4, 8) if 256 * n >= C) and last == C // 4 - 64 * (-(-C // 256) - 1)
    # the stem
    e = re.search(r"E % (\d+) == 0 and (\d+) <= E <= (\d+)", doc("adm_patch_embed_ln_fwd"))
    es = re.search(r"Supported E: E % (\d+) == 0, (\d+) <= E <= (\d+)", SOURCE)
    em = re.search(r"E % (\d+) == 0, (\d+) <= E <= PE_MAXE", SOURCE)
    maxe = re.search(r"#define PE_MAXE (\d+)", SOURCE)
    assert e and es and em and maxe and e.groups() == es.groups() == em.groups() + (maxe.group(1),)
    estep, elo, ehi = (int(v) for v in e.groups())
    for E in range(1, 600):
        assert (sc.pe_form(E) is not None) == (elo <= E <= ehi and E % estep == 0), E
    line = re.search(r"// G lanes per token, Q float4 per lane: (.*)\n#define PE_DISPATCH", SOURCE).group(1)
    assert line == "32 -> (8, 1), 64 -> (16, 1), 96 / 128 -> (32, 1), 160 .. 256 -> (64, 1), above -> (64, 2)"
    said = {32: (8, 1), 64: (16, 1), 96: (32, 1), 128: (32, 1)}
    said.update({E: (64, 1) for E in range(160, 257, 32)})
    said.update({E: (64, 2) for E in range(288, ehi + 1, 32)})
    assert sorted(said) == list(range(elo, ehi + 1, estep))
    for E, gq in said.items():
        assert sc.pe_form(E) == gq + (E // 4,), E
    # "G = the power of two >= E / 4 (at most 64)"
    assert "G = the power of two >= E / 4 (at most 64)" in SOURCE
    for E in said:
        g = 1
        while g < E // 4:
            g *= 2
        assert sc.pe_form(E)[0] == min(g, 64)
