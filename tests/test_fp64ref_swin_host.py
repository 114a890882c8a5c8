"""CPU-only: the fp64 references of the Swin encoder kernels (tests/fp64ref.py: layer_norm_affine, merge_layer_norm,
window_attention, patch_embed_ln, row_scale_add) and the bar tests/test_hip_swin_forms.py holds the kernels to.

(a) each reference equals fp64 autograd over tests/swin_ref.py / tests/swin_sci_ref.py (whose arithmetic the goldens pin to the
    reference's own classes) on the tables of tests/swin_cases.py;
(b) an fp32 model of the LayerNorm kernels' own arithmetic (shift by the row's first element, two passes) is inside bar A on every row
    class, while fp32 torch.layer_norm is not -- so the LayerNorm limit is bar A flat; plain fp32 torch is under
    swin_cases.F32_TORCH_CEILING on every attention and stem case, so max(bar A, 2 x fp32 torch) is bar A there;
(c) the bar rejects each defect of swin_cases.*_DEFECTS (an otherwise exact fp64 implementation with the defect) on the listed cases.
"""
import pytest
import torch

import fp64ref
import swin_cases as sc
import swin_ref as R
import swin_sci_ref as S

f64 = torch.float64
TIGHT = 1e-10          # fp64 against fp64, relative to max mag (the -1000 rows cost either side 1e3 x 1.1e-16 before rstd scales it)


def _same(ref, other, names=None):
    for n in names or ref:
        e = fp64ref.errors(other[n], *ref[n])[0]
        assert e <= TIGHT, (n, e)
        assert float(ref[n][1].min()) >= 0.0 and bool((ref[n][1] + 1e-300 >= ref[n][0].abs() * (1 - 1e-9)).all()), n      # mag bounds |ref|


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("case", [c for c in sc.LN_CASES if c[0] == 37], ids=str)
def test_layer_norm_reference_matches_autograd(case):
    x, w, b, dy = sc.ln_data(case)
    _same(sc.ln_reference(case), sc.torch_ln(x, w, b, dy, f64))


@pytest.mark.parametrize("case", [c for c in sc.MERGE_CASES if sc.merge_rows(c) < 1000], ids=str)
def test_merge_reference_matches_autograd(case):
    x, w, b, dy = sc.merge_data(case)
    xr, wr, br = (t.to(f64).requires_grad_(True) for t in (x, w, b))
    y = R.merge_ln(xr, wr, br)
    g = torch.autograd.grad(y, (xr, wr, br), dy.to(f64))
    want = {"y": y.detach(), "dx": g[0], "dw": g[1], "db": g[2]}
    _same(sc.merge_reference(case), want)
    _same(sc.merge_reference(case), sc.torch_ln(x, w, b, dy, f64, merge=True))
    assert torch.equal(sc.gathered(case, x), R.merge_gather(x).reshape(-1, 4 * case[3]))


@pytest.mark.parametrize("case", sc.ATTN_CASES, ids=sc.attn_id)
def test_window_attention_reference_matches_autograd(case):
    qkv, bias, table, dout = sc.attn_data(case)
    heads, (sh, sw) = case.geom[3], case.geom[4]
    ref = sc.attn_reference(case)
    _same(ref, sc.torch_attention(qkv, bias, table, heads, (sh, sw), dout, f64))
    if sh == sw:          # swin_ref.attn_core takes one shift for both axes
        q, b, t = (u.to(f64).requires_grad_(True) for u in (qkv, bias, table))
        out = R.attn_core(q, b, t, heads, sh)
        g = torch.autograd.grad(out, (q, b, t), dout.to(f64))
        _same(ref, {"out": out.detach(), "d_qkv": g[0], "d_qkv_bias": g[1], "d_table": g[2]})
    C = 32 * heads
    assert float(ref["d_qkv_bias"][0][:C].abs().max()) == 0.0 and float(ref["d_qkv_bias"][1][:C].abs().max()) == 0.0
    if sc.attn_padded(case.geom):
        assert float(ref["d_qkv_bias"][0][C:2 * C].abs().max()) > 0 and float(ref["d_qkv_bias"][0][2 * C:].abs().max()) > 0
    else:
        assert float(ref["d_qkv_bias"][0].abs().max()) == 0.0


def test_window_index_with_unequal_shifts_is_the_roll_and_partition():
    """fp64ref.window_index against the reference's own chain (pad, roll by (-sh, -sw), cut into windows) on a map of coordinates."""
    for H, W, shift in ((13, 8, (2, 5)), (6, 20, (6, 1)), (15, 7, (3, 3)), (9, 10, (3, 3))):
        Y, X, lab, _, (sh, sw) = fp64ref.window_index(H, W, shift)
        Ph, Pw = -(-H // 7) * 7, -(-W // 7) * 7
        yy, xx = torch.meshgrid(torch.arange(Ph), torch.arange(Pw), indexing="ij")
        win = lambda t: torch.roll(t, (-sh, -sw), (0, 1)).reshape(Ph // 7, 7, Pw // 7, 7).permute(0, 2, 1, 3).reshape(-1, 49)
        assert torch.equal(win(yy), Y) and torch.equal(win(xx), X)
        # the reference's mask: slices (0, -7), (-7, -shift), (-shift, None) of the rolled frame, numbered row-major
        img = torch.zeros(Ph, Pw, dtype=torch.long)
        cnt = 0
        for hs in ((0, Ph - 7), (Ph - 7, Ph - sh), (Ph - sh, Ph)):
            for ws in ((0, Pw - 7), (Pw - 7, Pw - sw), (Pw - sw, Pw)):
                img[hs[0]:hs[1], ws[0]:ws[1]] = cnt
                cnt += 1
        m = img.reshape(Ph // 7, 7, Pw // 7, 7).permute(0, 2, 1, 3).reshape(-1, 49)
        if sh + sw > 0:
            assert torch.equal(m[:, :, None] != m[:, None, :], lab[:, :, None] != lab[:, None, :]), (H, W, shift)


@pytest.mark.parametrize("case", [c for c in sc.STEM_CASES if sc.pe_tokens(c.geom) < 1000], ids=sc.stem_id)
def test_stem_reference_matches_autograd(case):
    x, dy = sc.stem_data(case)
    _same(sc.stem_reference(case), sc.torch_stem(x, *sc.stem_params(case.E), dy, f64))


def test_row_scale_add_reference():
    for case in sc.ROWSCALE_CASES:
        x, r, s = sc.rowscale_data(case)
        y = fp64ref.row_scale_add(x, r, s)["y"][0]
        assert torch.equal(y, x.double() + s.double()[:, None] * r.double())          # (x + 0 * r == x in value)
        drop = s == 0
        assert torch.equal(y[drop].to(torch.float32).view(torch.int32), x[drop].view(torch.int32))
        g = fp64ref.row_scale_add(None, r, s)["y"][0]
        assert torch.equal(g, s.double()[:, None] * r.double()) and not bool(torch.signbit(g[drop]).any())


# ------------------------------------------------------------------------------------------------ (b)
def _kernel_model_f32(x, w, b):
    """The LayerNorm kernels' arithmetic in fp32: sums of x - x0 (x0 the row's first element), then squared deviations from the mean."""
    C = x.shape[-1]
    v = x - x[..., :1]
    mean = v.sum(dim=-1, keepdim=True) / C
    d = v - mean
    rstd = 1.0 / torch.sqrt(d.square().sum(dim=-1, keepdim=True) / C + sc.EPS)
    return d * rstd * w + b


def test_layer_norm_limit_is_bar_a_flat():
    """Per row class: the kernel's own arithmetic in fp32 is far inside bar A; fp32 torch.layer_norm is outside it on the offset rows,
    so 2 x fp32 torch would hide a loss of the shifted statistics."""
    worst_model, worst_torch = {}, {}
    for case in (c for c in sc.LN_CASES if c[0] == 37):
        x, w, b, _ = sc.ln_data(case)
        ref = sc.ln_reference(case)["y"]
        for c, e in sc.class_errors(_kernel_model_f32(x, w, b), *ref).items():
            worst_model[c] = max(worst_model.get(c, 0.0), e[0])
        for c, e in sc.class_errors(R.layer_norm(x, w, b), *ref).items():
            worst_torch[c] = max(worst_torch.get(c, 0.0), e[0])
    print("kernel model:", {c: f"{v:.1e}" for c, v in worst_model.items()})
    print("fp32 torch:  ", {c: f"{v:.1e}" for c, v in worst_torch.items()})
    assert max(worst_model.values()) <= 1e-6
    assert worst_model["const"] == 0.0
    assert max(worst_torch["+300"], worst_torch["-1000"], worst_torch["300+1e-2u"]) > sc.BAR_A


@pytest.mark.parametrize("case", sc.ATTN_CASES, ids=sc.attn_id)
def test_fp32_torch_attention_is_under_the_ceiling(case):
    e = sc.attn_e32(case)
    print(sc.attn_id(case), {n: f"{v:.2e}" for n, v in e.items()})
    for n, v in e.items():
        assert v <= sc.F32_TORCH_CEILING, (n, v)
        assert sc.attn_limit(case, n) == sc.BAR_A


@pytest.mark.parametrize("case", [c for c in sc.STEM_CASES if c.geom[1] < 700], ids=sc.stem_id)
def test_fp32_torch_stem_is_under_the_ceiling(case):
    e = sc.stem_e32(case)
    print(sc.stem_id(case), {n: f"{v:.2e}" for n, v in e.items()})
    for n, v in e.items():
        assert v <= sc.F32_TORCH_CEILING, (n, v)
        assert sc.stem_limit(case, n) == sc.BAR_A


# ------------------------------------------------------------------------------------------------ (c)
def _ln_missed(got, ref):
    """Outputs that miss bar A: y and dx per row class, dw and db over the tensor (a NaN misses it too)."""
    missed = []
    for n in ("y", "dx"):
        for c, e in sc.class_errors(got[n], *ref[n]).items():
            if not e[0] <= sc.BAR_A:
                missed.append((n, c, e[0]))
    for n in ("dw", "db"):
        e = fp64ref.errors(got[n], *ref[n])
        if not e[0] <= sc.BAR_A:
            missed.append((n, None, e[0]))
    return missed


@pytest.mark.parametrize("defect", sc.LN_DEFECTS)
def test_bar_rejects_layer_norm_defect(defect):
    """On every M = 37 case (the eps defects: decided by the tiny rows; the divisor: by every class but the constant row)."""
    for case in (c for c in sc.LN_CASES if c[0] == 37):
        x, w, b, dy = sc.ln_data(case)
        assert not _ln_missed(sc.torch_ln(x, w, b, dy, f64), sc.ln_reference(case))
        missed = _ln_missed(sc.torch_ln(x, w, b, dy, f64, defect=defect), sc.ln_reference(case))
        print(case, defect, [(n, c, f"{v:.1e}") for n, c, v in missed][:6])
        assert missed, case
        if defect.startswith("eps"):
            assert any(n == "y" and c == "tiny" for n, c, _ in missed), case


def test_eps_is_decided_by_the_tiny_rows_only():
    """A dropped eps moves a plain row by about 2e-5 of mag -- inside the suite's older bar (rtol 1e-3) -- and a tiny row by O(1)."""
    case = (37, 2048)
    x, w, b, dy = sc.ln_data(case)
    e = sc.class_errors(sc.torch_ln(x, w, b, dy, f64, defect="eps dropped")["y"], *sc.ln_reference(case)["y"])
    print({c: f"{v[0]:.1e}" for c, v in e.items()})
    assert e["plain"][0] < 1e-4 and e["tiny"][0] > 1.0


@pytest.mark.parametrize("defect", sc.MERGE_DEFECTS)
def test_bar_rejects_merge_defect(defect):
    """On every (2, 9, 11, Cin) case: odd on both axes, so both the quad order and the padded positions show."""
    for case in (c for c in sc.MERGE_CASES if c[1:3] == (9, 11)):
        x, w, b, dy = sc.merge_data(case)
        ref = sc.merge_reference(case)
        flat = lambda r: {n: (sc.gathered(case, v) if n == "dx" else v) for n, v in r.items()}
        refg = {n: tuple(sc.gathered(case, t) if n == "dx" else t for t in v) for n, v in ref.items()}
        assert not _ln_missed(flat(sc.torch_ln(x, w, b, dy, f64, merge=True)), refg)
        missed = _ln_missed(flat(sc.torch_ln(x, w, b, dy, f64, defect=defect, merge=True)), refg)
        print(case, defect, [(n, c, f"{v:.1e}") for n, c, v in missed][:6])
        assert any(n == "y" for n, _, _ in missed) and any(n == "dx" for n, _, _ in missed), case


_SHIFTED = [c for c in sc.ATTN_CASES if fp64ref.window_index(c.geom[1], c.geom[2], c.geom[4])[4] != (0, 0)]
_PADDED = [c for c in sc.ATTN_CASES if sc.attn_padded(c.geom)]
_MANY = [c for c in sc.ATTN_CASES if c.geom[1] * c.geom[2] > 1]          # (one real token among 48 equal bias keys shows neither the scale nor the table's order)
ATTN_TEETH = [
    (sc.ATTN_DEFECTS[0], _SHIFTED, None),
    (sc.ATTN_DEFECTS[1], _MANY, None),
    (sc.ATTN_DEFECTS[2], _MANY, None),
    (sc.ATTN_DEFECTS[3], _MANY, None),
    (sc.ATTN_DEFECTS[4], _PADDED, "out"),
    (sc.ATTN_DEFECTS[5], _PADDED, "d_qkv_bias"),
]


def test_every_attention_defect_has_a_row():
    assert [t[0] for t in ATTN_TEETH] == list(sc.ATTN_DEFECTS) and all(t[1] for t in ATTN_TEETH)


@pytest.mark.parametrize("defect,cases,output", ATTN_TEETH, ids=[t[0].replace(" ", "-") for t in ATTN_TEETH])
def test_bar_rejects_attention_defect(defect, cases, output):
    for case in cases:
        qkv, bias, table, dout = sc.attn_data(case)
        bad = sc.torch_attention(qkv, bias, table, case.geom[3], case.geom[4], dout, f64, defect=defect)
        ref = sc.attn_reference(case)
        e = {n: fp64ref.errors(bad[n], *ref[n])[0] for n in ref}
        missed = [n for n in ref if not e[n] <= sc.attn_limit(case, n)]
        print(sc.attn_id(case), defect, {n: f"{v:.1e}" for n, v in e.items()})
        assert missed, (sc.attn_id(case), e)
        if output is not None:
            assert output in missed, (sc.attn_id(case), e)


def test_bar_rejects_stem_mean_over_the_lanes():
    """Every E whose row does not fill its G Q lanes (96, 160, 192, 288, 384), on both small images, plain and offset content."""
    seen = set()
    for case in (c for c in sc.STEM_CASES if c.geom in sc.STEM_SMALL and c.content != "zero"):
        g, q, e4 = sc.pe_form(case.E)
        if g * q == e4:
            continue
        seen.add(case.E)
        x, dy = sc.stem_data(case)
        bad = sc.torch_stem(x, *sc.stem_params(case.E), dy, f64, defect=sc.STEM_DEFECTS[0], lanes=4.0 * g * q)
        ref = sc.stem_reference(case)
        e = {n: fp64ref.errors(bad[n], *ref[n])[0] for n in ref}
        print(sc.stem_id(case), {n: f"{v:.1e}" for n, v in e.items()})
        assert not e["y"] <= sc.stem_limit(case, "y"), (sc.stem_id(case), e)
    assert seen == {96, 160, 192, 288, 384}
