"""GPU: every compiled form of the Swin encoder kernels (csrc/swin.hip) against fp64, through the C ABI.

tests/swin_cases.py holds the tables; tests/test_swin_cases_host.py shows on the CPU that they reach every (MERGE, NQ) form of the
LayerNorm kernels whole and partial, every (G, Q) lane layout of the stem with and without lanes past the row, and both sides of the
two backward grids' caps; tests/test_fp64ref_swin_host.py pins the references and shows what the bar rejects.

Every case runs forward and backward twice into fresh sentinel-filled outputs: the second run equals the first bit for bit, no
sentinel is left in an output, the 4 KB guards around y / dx / out / d_qkv and after the exactly-sized workspace stay intact.  Limits,
relative to the same sums over |summands| (fp64ref.errors):

  LayerNorm, plain and merged   bar A (e_max <= 1e-5) flat; y and dx PER ROW CLASS (swin_cases.class_errors), dw and db over the tensor
  window attention, the stem    max(bar A, 2 x e_max of fp32 torch on the same data) = swin_cases.attn_limit / stem_limit -- which is
                                bar A on every case of the tables (test_fp64ref_swin_host.py: fp32 torch stays under 5e-6)
  rowscale_add                  the bits of one fused multiply-add

Then the accumulate flags of the three backward entry points, the unaligned image, and the worst errors per kernel, form and output.
"""
import pytest
import torch

import fp64ref
import swin_cases as sc

pytestmark = pytest.mark.gpu

WORST = {}        # (kernel, form, output) -> [e_max, e_rms]
SENTINEL = -12345.5
GUARD = 1024      # floats: 4 KB


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip as _hip
    _hip.lib()        # raises if the HIP library is missing: no fallback
    return _hip


def _guarded(n):
    """(whole buffer, payload view of n floats): sentinel everywhere, GUARD floats on either side of the payload."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _workspace(n):
    """A workspace of exactly n floats with a guard after it."""
    return torch.full((n + GUARD,), SENTINEL, device="cuda")


def _written(t):
    return bool((t != SENTINEL).all()) and bool(torch.isfinite(t).all())


def _note(kernel, form, out, e):
    w = WORST.setdefault((kernel, form, out), [0.0, 0.0])
    w[0], w[1] = max(w[0], e[0]), max(w[1], e[1])


def _cuda(ts):
    return tuple(t.cuda() for t in ts)


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_run(hip, merge, case, dev, acc=0, dw=None, db=None):
    """One forward and one backward of a plain (M, C) or merged (B, H, W, Cin) case.  {"y", "dx", "dw", "db"}; guards checked."""
    x, w, b, dy = dev
    p = hip.ptr
    if merge:
        B, H, W, Cin = case
        M, C = sc.merge_rows(case), 4 * Cin
    else:
        M, C = case
    ybuf, y = _guarded(M * C)
    dxbuf, dx = _guarded(x.numel())
    dw = torch.full((C,), SENTINEL, device="cuda") if dw is None else dw
    db = torch.full((C,), SENTINEL, device="cuda") if db is None else db
    n_ws = hip.lib().adm_ln_bwd_ws_floats(M, C)
    assert n_ws == sc.ln_bwd_blocks(M, C) * sc.LN_ROWS * 2 * C > 0
    ws = _workspace(n_ws)
    if merge:
        hip.call("adm_swin_merge_ln_fwd", p(x), p(w), p(b), p(y), B, H, W, Cin, sc.EPS)
        hip.call("adm_swin_merge_ln_bwd", p(x), p(w), p(dy), p(dx), p(dw), p(db), p(ws), B, H, W, Cin, sc.EPS, acc)
    else:
        hip.call("adm_ln_affine_fwd", p(x), p(w), p(b), p(y), M, C, sc.EPS)
        hip.call("adm_ln_affine_bwd", p(x), p(w), p(dy), p(dx), p(dw), p(db), p(ws), M, C, sc.EPS, acc)
    torch.cuda.synchronize()
    assert _intact(ybuf) and _intact(dxbuf) and bool((ws[n_ws:] == SENTINEL).all()), "a write outside y, dx or the workspace"
    return {"y": y.reshape(M, C), "dx": dx.reshape(x.shape), "dw": dw, "db": db}


def _ln_check(hip, merge, case, data, ref):
    dev = _cuda(data)
    got, again = _ln_run(hip, merge, case, dev), _ln_run(hip, merge, case, dev)
    M, C = got["y"].shape
    form = sc.ln_label(merge, C) + ("" if sc.ln_bwd_blocks(M, C) < sc.LN_BWD_MAXBLOCKS else ":capped")
    bad = []
    for n in ("y", "dx", "dw", "db"):
        assert torch.equal(got[n], again[n]), f"{n}: the second run differs"
        assert _written(got[n]), f"{n}: an element was left unwritten or is not finite"
    if merge:          # dx per class of the row it came from: back through the gather
        got = dict(got, dx=sc.gathered(case, got["dx"]))
        ref = dict(ref, dx=tuple(sc.gathered(case, t) for t in ref["dx"]))
    for n, kernel in (("y", "ln_fwd"), ("dx", "ln_bwd")):
        for c, e in sc.class_errors(got[n], *ref[n]).items():
            _note(kernel, form, f"{n}[{c}]", e)
            print(f"{case} {form} {n:2s} {c:10s} e_max {e[0]:.3e} e_rms {e[1]:.3e}")
            if not e[0] <= sc.BAR_A:
                bad.append(f"{n} [{c}] e_max {e[0]:.3e} > {sc.BAR_A:.0e}")
    for n in ("dw", "db"):
        e = fp64ref.errors(got[n], *ref[n])
        _note("ln_bwd", form, n, e)
        print(f"{case} {form} {n:2s} {'':10s} e_max {e[0]:.3e} e_rms {e[1]:.3e}")
        if not e[0] <= sc.BAR_A:
            bad.append(f"{n} e_max {e[0]:.3e} > {sc.BAR_A:.0e}")
    # the constant row: x - x0 = 0 everywhere, so y is the bias to the bit
    if M > 7 and (not merge or bool(sc.merge_whole_rows(case)[7])):
        assert torch.equal(got["y"][7], dev[2]), "the constant row's y is not the bias"
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", sc.LN_CASES, ids=lambda c: f"M{c[0]}-C{c[1]}")
def test_layer_norm_forms_vs_fp64(hip, case):
    _ln_check(hip, False, case, sc.ln_data(case), sc.ln_reference(case))


@pytest.mark.parametrize("case", sc.MERGE_CASES, ids=lambda c: f"B{c[0]}-{c[1]}x{c[2]}-Cin{c[3]}")
def test_merge_layer_norm_forms_vs_fp64(hip, case):
    _ln_check(hip, True, case, sc.merge_data(case), sc.merge_reference(case))


@pytest.mark.parametrize("merge,case", [(False, (37, 260)), (False, (4099, 32)), (True, (2, 9, 11, 24))])
def test_layer_norm_accumulate(hip, merge, case):
    """accumulate = 1 onto pre-filled dw / db: the prefill plus the fresh result (one fp32 addition), dx as without it."""
    dev = _cuda(sc.merge_data(case) if merge else sc.ln_data(case))
    fresh = _ln_run(hip, merge, case, dev)
    C = fresh["dw"].numel()
    pre_w, pre_b = torch.linspace(-3.0, 5.0, C, device="cuda"), torch.linspace(100.0, -100.0, C, device="cuda")
    acc = _ln_run(hip, merge, case, dev, acc=1, dw=pre_w.clone(), db=pre_b.clone())
    assert torch.equal(acc["dw"], pre_w + fresh["dw"]) and torch.equal(acc["db"], pre_b + fresh["db"])
    assert torch.equal(acc["dx"], fresh["dx"]) and torch.equal(acc["y"], fresh["y"])


# ------------------------------------------------------------------------------------------------ window attention
def _attn_run(hip, case, dev, acc_table=0, acc_bias=0, d_table=None, d_bias=None):
    qkv, bias, table, dout = dev
    B, H, W, heads, (sh, sw) = case.geom
    C = 32 * heads
    p = hip.ptr
    obuf, out = _guarded(B * H * W * C)
    gbuf, d_qkv = _guarded(qkv.numel())
    d_table = torch.full((169, heads), SENTINEL, device="cuda") if d_table is None else d_table
    d_bias = torch.full((3 * C,), SENTINEL, device="cuda") if d_bias is None else d_bias
    n_ws = hip.lib().adm_swin_attn_bwd_ws_floats(B, H, W, heads)
    assert n_ws == sc.attn_units(case.geom) * 240
    ws = _workspace(n_ws)
    hip.call("adm_swin_attn_fwd", p(qkv), p(bias), p(table), p(out), B, H, W, C, heads, 7, sh, sw)
    hip.call("adm_swin_attn_bwd", p(qkv), p(bias), p(table), p(dout), p(d_qkv), p(d_table), p(d_bias), p(ws), B, H, W, C, heads, 7, sh, sw,
             acc_table, acc_bias)
    torch.cuda.synchronize()
    assert _intact(obuf) and _intact(gbuf) and bool((ws[n_ws:] == SENTINEL).all()), "a write outside out, d_qkv or the workspace"
    return {"out": out.reshape(B, H, W, C), "d_qkv": d_qkv.reshape(qkv.shape), "d_table": d_table, "d_qkv_bias": d_bias}


@pytest.mark.parametrize("case", sc.ATTN_CASES, ids=sc.attn_id)
def test_window_attention_vs_fp64(hip, case):
    dev = _cuda(sc.attn_data(case))
    got, again = _attn_run(hip, case, dev), _attn_run(hip, case, dev)
    ref = sc.attn_reference(case)
    C = 32 * case.geom[3]
    bad = []
    for n, kernel in (("out", "attn_fwd"), ("d_qkv", "attn_bwd"), ("d_table", "attn_bwd"), ("d_qkv_bias", "attn_bwd")):
        assert torch.equal(got[n], again[n]), f"{n}: the second run differs"
        assert _written(got[n]), f"{n}: an element was left unwritten or is not finite"
        e, lim = fp64ref.errors(got[n], *ref[n]), sc.attn_limit(case, n)
        _note(kernel, case.kind, n, e)
        print(f"{sc.attn_id(case)} {n:10s} e_max {e[0]:.3e} e_rms {e[1]:.3e} limit {lim:.1e}")
        if not e[0] <= lim:
            bad.append(f"{n} e_max {e[0]:.3e} > {lim:.3e}")
    assert float(got["d_qkv_bias"][:C].abs().max()) == 0.0, "a padding token is never a query: the q third of d_qkv_bias is zero"
    if sc.attn_padded(case.geom):          # the padding keys' dK and dV arrive (where fp64 has them above the bar: one real token
        rb, mb = ref["d_qkv_bias"]         # under a +-20 table leaves the 48 equal bias keys a dK of 1e-9 of mag, 0 in fp32)
        for third in (slice(C, 2 * C), slice(2 * C, 3 * C)):
            if float(rb[third].abs().max()) > sc.BAR_A * float(mb.max()):
                assert float(got["d_qkv_bias"][third].abs().max()) > 0
    else:
        assert float(got["d_qkv_bias"].abs().max()) == 0.0
    assert not bad, "\n".join(bad)


def test_window_attention_accumulate_flags(hip):
    """acc_table and acc_bias each alone onto pre-filled destinations; with acc_bias the q third stays as it was."""
    case = sc.AttnCase(sc.ATTN_GEOM[0], "hashed")
    assert sc.attn_padded(case.geom)
    dev = _cuda(sc.attn_data(case))
    heads = case.geom[3]
    C = 32 * heads
    fresh = _attn_run(hip, case, dev)
    pre_t = torch.linspace(-2.0, 2.0, 169 * heads, device="cuda").reshape(169, heads)
    pre_b = torch.linspace(7.0, -7.0, 3 * C, device="cuda")
    a = _attn_run(hip, case, dev, acc_table=1, d_table=pre_t.clone())
    assert torch.equal(a["d_table"], pre_t + fresh["d_table"]) and torch.equal(a["d_qkv_bias"], fresh["d_qkv_bias"])
    b = _attn_run(hip, case, dev, acc_bias=1, d_bias=pre_b.clone())
    assert torch.equal(b["d_table"], fresh["d_table"])
    assert torch.equal(b["d_qkv_bias"][C:], pre_b[C:] + fresh["d_qkv_bias"][C:]) and torch.equal(b["d_qkv_bias"][:C], pre_b[:C])
    for r in (a, b):
        assert torch.equal(r["d_qkv"], fresh["d_qkv"]) and torch.equal(r["out"], fresh["out"])


# ------------------------------------------------------------------------------------------------ the stem
def _stem_run(hip, geom, E, x, dy, params, acc=0, grads=None):
    B, H, W = geom
    w, cb, gamma, beta = params
    p = hip.ptr
    T = sc.pe_tokens(geom)
    ybuf, y = _guarded(T * E)
    names = ("dW", "db", "dgamma", "dbeta")
    if grads is None:
        grads = {n: torch.full((16 * E if n == "dW" else E,), SENTINEL, device="cuda") for n in names}
    n_ws = hip.lib().adm_patch_embed_ln_bwd_ws_floats(B, H, W, E)
    assert n_ws == sc.pe_bwd_blocks(geom, E) * sc.PE_PART * E > 0
    ws = _workspace(n_ws)
    hip.call("adm_patch_embed_ln_fwd", p(x), p(w), p(cb), p(gamma), p(beta), p(y), B, H, W, E, sc.EPS)
    hip.call("adm_patch_embed_ln_bwd", p(x), p(w), p(cb), p(gamma), p(dy), *(p(grads[n]) for n in names), p(ws), B, H, W, E, sc.EPS, acc)
    torch.cuda.synchronize()
    assert _intact(ybuf) and bool((ws[n_ws:] == SENTINEL).all()), "a write outside y or the workspace"
    out = dict(grads, y=y.reshape(B, H // 4, W // 4, E))
    out["dW"] = out["dW"].reshape(E, 1, 4, 4)
    return out


STEM_RUNS = [(g, E) for E in sc.STEM_E for g in sc.STEM_SMALL] + list(sc.STEM_CAPPED)


@pytest.mark.parametrize("geom,E", STEM_RUNS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"E{v}")
def test_stem_forms_vs_fp64(hip, geom, E):
    """Every content of the (image, E) pair in swin_cases.STEM_CASES."""
    params = _cuda(sc.stem_params(E))
    form = sc.pe_label(E) + ("" if sc.pe_bwd_blocks(geom, E) < sc.PE_BWD_MAXBLOCKS else ":capped")
    cases = [c for c in sc.STEM_CASES if c.geom == geom and c.E == E]
    assert cases
    bad = []
    for case in cases:
        x, dy = _cuda(sc.stem_data(case))
        got, again = _stem_run(hip, geom, E, x, dy, params), _stem_run(hip, geom, E, x, dy, params)
        ref = sc.stem_reference(case)
        for n in ref:
            assert torch.equal(got[n], again[n]), f"{case.content} {n}: the second run differs"
            assert _written(got[n]), f"{case.content} {n}: an element was left unwritten or is not finite"
            e, lim = fp64ref.errors(got[n], *ref[n]), sc.stem_limit(case, n)
            _note("stem_fwd" if n == "y" else "stem_bwd", form, f"{n}[{case.content}]", e)
            print(f"{sc.stem_id(case)} {form} {n:6s} e_max {e[0]:.3e} e_rms {e[1]:.3e} limit {lim:.1e}")
            if not e[0] <= lim:
                bad.append(f"{case.content} {n} e_max {e[0]:.3e} > {lim:.3e}")
        if case.content == "zero":
            # every token's conv output is the conv bias: all rows are the same row; without a conv bias every deviation is 0 and y
            # is the LayerNorm bias to the bit
            y = got["y"]
            assert torch.equal(y, y[:1, :1, :1].expand_as(y))
            nob = _stem_run(hip, geom, E, x, dy, (params[0], torch.zeros_like(params[1]), params[2], params[3]))
            assert torch.equal(nob["y"], params[3].expand_as(y))
    assert not bad, "\n".join(bad)


def test_stem_unaligned_image(hip):
    """x offset by 4 bytes with W % 4 == 0: alignment alone sends the patch load down the by-element path; the same bits."""
    geom, E = (2, 8, 12), 96
    B, H, W = geom
    params = _cuda(sc.stem_params(E))
    x, dy = _cuda(sc.stem_data(sc.StemCase(geom, E, "plain")))
    buf = torch.zeros(x.numel() + 1, device="cuda")
    xo = buf[1:]
    xo.copy_(x.reshape(-1))
    assert x.data_ptr() % 16 == 0 and xo.data_ptr() % 16 == 4
    a, b = _stem_run(hip, geom, E, x, dy, params), _stem_run(hip, geom, E, xo, dy, params)
    ref = fp64ref.patch_embed_ln(x, *params, sc.EPS, dy)
    for n in ref:
        assert torch.equal(a[n], b[n]), n
        assert fp64ref.errors(b[n], *ref[n])[0] <= sc.BAR_A, n


def test_stem_accumulate_bits(hip):
    """Each of the four accumulate bits alone: that destination is the prefill plus the fresh result, the other three are fresh."""
    geom, E = (2, 30, 46), 160
    params = _cuda(sc.stem_params(E))
    x, dy = _cuda(sc.stem_data(sc.StemCase(geom, E, "plain")))
    names = ("dW", "db", "dgamma", "dbeta")
    fresh = _stem_run(hip, geom, E, x, dy, params)
    for bit, which in enumerate(names):
        pre = {n: torch.linspace(-4.0, 9.0, 16 * E if n == "dW" else E, device="cuda") for n in names}
        got = _stem_run(hip, geom, E, x, dy, params, acc=1 << bit, grads={n: t.clone() for n, t in pre.items()})
        for n in names:
            want = pre[n] + fresh[n].reshape(-1) if n == which else fresh[n].reshape(-1)
            assert torch.equal(got[n].reshape(-1), want), (which, n)


# ------------------------------------------------------------------------------------------------ rowscale_add
@pytest.mark.parametrize("case", sc.ROWSCALE_CASES, ids=lambda c: f"B{c[0]}-n{c[1]}")
def test_rowscale_add_bits(hip, case):
    """y = fma(s, r, x) and, without x, y = s r: the fp64 value rounded once to fp32, bit for bit; a sample with s == 0 is x (even
    the sign of a zero) or +0."""
    B, n = case
    x, r, s = sc.rowscale_data(case)
    xd, rd, sd = _cuda((x, r, s))
    p = hip.ptr
    bits = lambda t: t.cpu().view(torch.int32)
    for with_x in (True, False):
        ybuf, y = _guarded(B * n)
        hip.call("adm_rowscale_add", p(xd) if with_x else None, p(rd), p(sd), p(y), B, n)
        torch.cuda.synchronize()
        assert _intact(ybuf)
        want = fp64ref.row_scale_add(x if with_x else None, r, s)["y"][0].to(torch.float32)
        assert torch.equal(bits(y.reshape(B, n)), bits(want)), with_x
        drop = s == 0
        assert bool(drop.any())
        if with_x:
            assert torch.equal(bits(y.reshape(B, n))[drop], bits(x)[drop])
        else:
            assert bool((bits(y.reshape(B, n))[drop] == 0).all())


def test_zz_report_worst_errors():
    """Worst e_max / e_rms per (kernel, form, output) over the sweep."""
    if not WORST:
        pytest.skip("no sweep ran in this session")
    print("\nworst error vs fp64 per kernel / form / output (e_max, e_rms):")
    for (kernel, form, out), (em, er) in sorted(WORST.items()):
        print(f"  {kernel:9s} {form:28s} {out:18s} {em:.3e} {er:.3e}")
