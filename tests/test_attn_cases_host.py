"""CPU-only: the table of the UNet attention sweep (tests/attn_cases.py) -- its conditioning, the forms it reaches, and the header.

adm_attn_form is the function through which dispatch_attn (attention.hip) and adm_attn_fwd_h3 / adm_attn_bwd_h3 (attention_h3.hip)
choose their instantiation, so what it answers is what runs.  This file shows that the plain fp32 torch restatement alone is inside the
limits the kernels are held to in tests/test_hip_attention_forms.py, that the table reaches every form the query can answer up to
L = 1024, that the lengths the sweep expects to be refused are refused, and that include/adm_hip.h's sentences on the supported L
say what the query says.
"""
import ctypes
import os
import re

import pytest

import attn_cases as ac
import fp64ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_is_declared_and_exported():
    from adm_amd import hip
    header = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    assert re.search(r"^int\s+adm_attn_form\s*\(int family, int L, int\* out\);", header, flags=re.M)
    assert "adm_attn_form" in hip.EXPORTS and "adm_attn_form" in hip.NO_STREAM
    lib, out = hip.lib(), (ctypes.c_int * 4)()
    assert lib.adm_attn_form(0, 64, None) == -22                                        # no output
    assert [lib.adm_attn_form(f, 64, out) for f in (-1, 3)] == [-22, -22]               # no such family
    assert [lib.adm_attn_form(f, L, out) for f in (0, 1, 2) for L in (0, -32)] == [-22] * 6
    assert lib.adm_attn_form(0, 65536, out) == 0 and lib.adm_attn_form(0, 65536 + 32, out) == -22
    assert lib.adm_attn_form(1, 16384, out) == 0 and lib.adm_attn_form(2, 16384 + 256, out) == -22


def test_table_shape():
    """What the sweep is meant to hold: the L values of each family, the modes of each, B <= 2, heads <= 3, both > 1 in each family."""
    hashed = {ac.seq_len(c): c for c in ac.CASES if c.kind == "hashed"}
    assert sorted(hashed) == [1, 9, 25, 32, 64, 96, 128, 160, 192, 224, 256, 288, 512, 576, 768]
    for L, c in hashed.items():
        assert c.modes == (ac.ALL_MODES if L in (32, 64, 128, 256, 512, 768) else ac.F32_MODES), L
    for fam in (ac.F32_MODES, ("h3", "h3-fwd")):
        geoms = [c.geom for c in ac.CASES if set(fam) <= set(c.modes)]
        assert any(g[0] > 1 for g in geoms) and any(g[3] > 1 for g in geoms)
    assert all(1 <= c.geom[0] <= 2 and 1 <= c.geom[3] <= 3 for c in ac.CASES)
    stairs = sorted((ac.seq_len(c), c.offsets) for c in ac.CASES if c.kind == "stair")
    assert stairs == [(512, (0, 12)), (768, (0, 25, 5)), (1024, (0, 10, 20, 30)), (1024, (30, 20, 10, 0))]
    assert all(c.modes == ac.ALL_MODES for c in ac.CASES if c.kind == "stair")
    assert all(c.geom[0] == 1 and c.geom[3] == 1 for c in ac.CASES if ac.seq_len(c) == 1024)
    assert {ac.seq_len(c) for c in ac.CASES if c.kind == "peaked"} >= {32, 128}
    assert len({ac.case_id(c) for c in ac.CASES}) == len(ac.CASES)


def test_stair_data_is_a_stair():
    """Channel 0 lifts every logit of a 256-key chunk by the chunk's offset: the running maximum of the online softmax moves by the
    steps of the list (the hashed part of a logit is a sum of 63 products / 8, |.| < 8)."""
    for c in (c for c in ac.CASES if c.kind == "stair"):
        qkv, _ = ac.data(c)
        B, H, W, heads = c.geom
        t = qkv.double().reshape(B, H * W, heads, 3, 64).permute(3, 0, 2, 1, 4)
        s = (t[0] @ t[1].transpose(-1, -2)) / 8.0                                     # [B][heads][q][key]
        base = s.clone()
        for i, off in enumerate(c.offsets):
            base[..., 256 * i:256 * (i + 1)] -= off
        assert float(base.abs().max()) < 4.0, ac.case_id(c)
        top = [float(s[..., 256 * i:256 * (i + 1)].max(dim=-1).values.min()) for i in range(len(c.offsets))]
        print(ac.case_id(c), "smallest per-query chunk maximum:", [f"{v:.1f}" for v in top])
        for (a, oa), (b, ob) in zip(zip(top, c.offsets), zip(top[1:], c.offsets[1:])):
            assert abs((b - a) - (ob - oa)) < 4.0


@pytest.mark.parametrize("case", ac.CASES, ids=ac.case_id)
def test_fp32_torch_is_inside_the_limit(case):
    """Reference conditioning: the fp32 torch restatement passes the limit the kernels are held to -- bar A on hashed data; on peaked and
    stair data it stays under F32_TORCH_CEILING, so that limit is bar A there too and 2 x the restatement never decides."""
    e = ac.e32(case)
    print(f"{ac.case_id(case)}: fp32 torch e_max out {e['out']:.2e} dqkv {e['dqkv']:.2e}")
    for out in ("out", "dqkv"):
        assert e[out] <= ac.limit(case, out)
        assert e[out] <= (ac.BAR_A if case.kind == "hashed" else ac.F32_TORCH_CEILING), (out, e)
        assert float(ac.reference(case)[out][1].max()) > 0
        assert ac.limit(case, out) == ac.BAR_A


def test_each_third_of_dqkv_holds_the_maximum_once():
    """The bound data: the named third of dqkv dominates the other two by more than the factor 8 of the 1/8 scale, so a bound taken
    before that scale, or without that third, cannot equal max |dqkv|."""
    for i, which in enumerate(("dq", "dk", "dv")):
        qkv, dout, heads = ac.bound_data(which)
        m = ac.third_maxima(fp64ref.attention(qkv, heads, dout)["dqkv"][0], heads)
        print(which, [f"{v:.3f}" for v in m])
        assert m[i] == max(m)
        if which != "dv":
            assert all(m[i] > 8.0 * v for j, v in enumerate(m) if j != i), (which, m)
        else:                                 # ... and here 8 max |dq| and 8 max |dk| would overshoot max |dv|
            assert 8.0 * m[0] > m[2] and 8.0 * m[1] > m[2], m


def _answerable(family, top=1024):
    return {ac.form_label(family, L) for L in range(1, top + 1)} - {None}


def test_sweep_reaches_every_form():
    """Every (family, form) the query can answer for L <= 1024 is run by a case of the table."""
    f32 = {"f32:1w-partial", "f32:8w-chunked-exact", "f32:8w-chunked-ragged"} | {f"f32:{w}w" for w in range(1, 9)}
    h3f = {"h3fwd:1w", "h3fwd:2w", "h3fwd:4w", "h3fwd:8w", "h3fwd:8w-chunked"}
    h3b = {"h3bwd:1w/32", "h3bwd:2w/64", "h3bwd:4w/128", "h3bwd:8w/128", "h3bwd:8w-chunked/128"}
    assert _answerable(0) == f32 and _answerable(1) == h3f and _answerable(2) == h3b
    assert ac.forms_reached() == f32 | h3f | h3b
    # the paths the issue names, by L
    assert [ac.form_label(0, L) for L in (1, 9, 25)] == ["f32:1w-partial"] * 3
    assert ac.form(0, 288) == (8, 256, 2, 1) and ac.form(0, 576) == (8, 256, 3, 1) and ac.form(0, 96) == (3, 96, 1, 0)
    assert ac.form(2, 32) == (1, 32, 1, 0) and ac.form(2, 128) == (4, 128, 1, 0) and ac.form(2, 256) == (8, 128, 1, 0)
    assert ac.form(1, 512) == (8, 256, 2, 1) and ac.form(2, 512) == (8, 128, 2, 1)
    # every h3 case also runs on the f32 family (bar B compares the two on the same data)
    assert all("f32" in c.modes for c in ac.CASES)


def test_refused_lengths():
    """What tests/test_hip_attention_forms.py expects to come back as ADM_EINVAL, and what ops.attention must therefore keep on the f32
    kernels."""
    assert [ac.form(0, L) for L in (33, 100, 144)] == [None] * 3
    assert [ac.form(f, L) for f in (1, 2) for L in (96, 320)] == [None] * 4
    assert ac.form(0, 96) is not None and ac.form(0, 320) is not None


def test_header_sentences_match_the_query():
    """include/adm_hip.h on the supported L of the two families, against adm_attn_form for L = 1..320."""
    header = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    doc = lambda name: re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+%s\s*\(" % name, header, flags=re.S).group(1)
    f32 = re.search(r"L <= (\d+) or a multiple of (\d+);", doc("adm_attn_fwd"))
    h3 = re.search(r"L in \{([\d, ]+)\} or a multiple of (\d+) \(ADM_EINVAL otherwise\)", doc("adm_attn_fwd_h3"))
    assert f32 and h3
    small, step = int(f32.group(1)), int(f32.group(2))
    listed, hstep = {int(v) for v in h3.group(1).split(",")}, int(h3.group(2))
    assert "L as above" in doc("adm_attn_bwd_h3")
    for L in range(1, 321):
        assert (ac.form(0, L) is not None) == (L <= small or L % step == 0), L
        for fam in (1, 2):
            assert (ac.form(fam, L) is not None) == (L in listed or L % hstep == 0), (fam, L)
