"""GPU: every kernel and tile form of the direct bf16 kernels (conv_igemm_bf16.hip, conv_wgrad_bf16.hip) against fp64.

The C entries are called through hip.call, so `tile` and `splits` can be forced at sizes of a few hundred pixels: the 128x128 and
128x96 forward forms and the unsplit / explicitly split weight gradients that production reaches only at batch 128
(tests/test_bf16_plan_host.py pins which).  The reference is fp64ref.conv on the operands ROUNDED as each kernel rounds them -- the
forward x and w, the data gradient dy and w, the weight gradient dy and x -- so what is measured is the kernel (indexing, epilogue,
accumulation), not the rounding.  Products of bf16 values are exact in fp32 and the MFMA accumulates in fp32:

  bar A   e_max <= 1e-5 (fp64ref.errors)                                   -- the project's bar for every path
  bar B   fp64ref.bar_b against the f32-MFMA kernel (adm_conv_fwd, adm_conv_wgrad_bias) run on the same rounded values

Besides the bars: rows past M and pad columns of a wide-stride output keep a NaN sentinel's bits; the stored-bf16 entry points
(adm_conv_fwd_bf16a, adm_conv_wgrad_bf16a) are bit-identical to the f32-input ones per form; a NaN-filled weight-gradient buffer
comes back finite in every element; the split modes follow the plan the host query gives.
"""
import ctypes

import pytest
import torch

import bf16_cases as bc
import fp64ref

pytestmark = pytest.mark.gpu

BAR_A = 1e-5
SENTINEL = 0x7FC0BEEF        # a quiet NaN with a payload: any store over it changes the bits
GUARD_ROWS = 64

WORST = {}                   # (kernel, form, output) -> [e_max, e_rms, worst bar-B ratio (max), (rms)]
RAN = set()                  # what the sweep executed: ("fwd", tile, stored) / ("wgrad", TM, TN, fast, stored, mode)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip as _hip
    _hip.lib()        # raises if the HIP library is missing: no fallback
    return _hip


def _note(kernel, form, out, e, ratios):
    w = WORST.setdefault((kernel, form, out), [0.0, 0.0, 0.0, 0.0])
    for i, v in enumerate((e[0], e[1]) + tuple(ratios)):
        w[i] = max(w[i], v)


def _sentinel(shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _judge(label, kernel, form, out, got, ref, e32, bad):
    """Errors of `got` against the fp64 (ref, mag), printed, noted for the report and held to bars A and B."""
    assert bool(torch.isfinite(got).all()), f"{label}: non-finite {out}"
    e = fp64ref.errors(got.cpu(), *ref)
    ok, rm, rr = fp64ref.bar_b(e, e32) if e32 is not None else (True, 0.0, 0.0)
    _note(kernel, form, out, e, (rm, rr))
    print(f"{label} {out}: e_max {e[0]:.2e} e_rms {e[1]:.2e}" + (f"  f32 {e32[0]:.2e}/{e32[1]:.2e}  ratios {rm:.2f}/{rr:.2f}" if e32 else ""))
    if e[0] > BAR_A:
        bad.append(f"bar A: {label} {out} e_max {e[0]:.3e} > {BAR_A}")
    if not ok:
        bad.append(f"bar B: {label} {out} e {e[0]:.3e}/{e[1]:.3e} vs f32 {e32[0]:.3e}/{e32[1]:.3e} (ratios {rm:.2f}, {rr:.2f})")
    return e


# ------------------------------------------------------------------------------------------------ weight operands
def test_weight_operand_layout_is_what_the_pack_kernels_produce(hip):
    """The sweep builds the bf16 operands in torch from the layout the kernels read (row n, column tap * Cin + c; the data gradient's with
    cin and cout exchanged and the taps flipped): bit-equal to adm_pack_weight + adm_f32_to_bf16, which is what ops feeds them."""
    for g in (bc.FWD[1], bc.FWD[2]):
        _, _, _, ci, co, ks, _ = g
        w = bc.data(g)["w"].cuda()
        fwd, bwd = torch.empty(co, ks * ks * ci, device="cuda"), torch.empty(ci, ks * ks * co, device="cuda")
        hip.call("adm_pack_weight", hip.ptr(w), hip.ptr(fwd), hip.ptr(bwd), co, ci, ks, co, ci, 0)
        for packed, mine in ((fwd, bc.fwd_operand(w)), (bwd, bc.bwd_operand(w))):
            assert torch.equal(packed, mine)
            p16 = torch.empty(packed.shape, device="cuda", dtype=torch.bfloat16)
            hip.call("adm_f32_to_bf16", hip.ptr(packed), hip.ptr(p16), packed.numel())
            torch.cuda.synchronize()
            assert torch.equal(p16.view(torch.int16), mine.to(torch.bfloat16).view(torch.int16))


# ------------------------------------------------------------------------------------------------ forward / data gradient
def _conv_launch(hip, sym, x, wop, bias, res, g, tile, ldy, ldr):
    """One launch of a forward entry point into a sentinel-filled [M + GUARD_ROWS][ldy] buffer; the whole buffer comes back."""
    B, H, W, ci, N, ks, up = g
    y = _sentinel((B * H * W + GUARD_ROWS, ldy))
    hip.call(sym, hip.ptr(x), hip.ptr(wop), hip.ptr(bias), hip.ptr(res), hip.ptr(y), B, H, W, ci, x.shape[-1], N, wop.shape[0], ldy, ldr, ks,
             up, tile)
    torch.cuda.synchronize()
    return y


def _check_untouched(y, M, N, label):
    yb = _bits(y)
    assert bool((yb[M:] == SENTINEL).all()), f"{label}: rows past M were written"
    if y.shape[1] > N:
        assert bool((yb[:M, N:] == SENTINEL).all()), f"{label}: pad columns were written"


def _sweep_conv(hip, label, g, x, w_op, bias, res, ref, out, ldy, bad, stored=(False, True)):
    """adm_conv_fwd_bf16 / _bf16a on every form at one geometry.  x: the un-rounded fp32 input (the f32 entry rounds it on load; the
    stored entry gets its bf16 values); w_op: the fp32 operand [rows][K] of rounded weights.  res has row stride ldy too."""
    B, H, W, ci, N, ks, up = g
    M = B * H * W
    x16 = x.to(torch.bfloat16)
    w16 = w_op.to(torch.bfloat16)
    y32 = _conv_launch(hip, "adm_conv_fwd", x16.to(torch.float32), w_op, bias, res, g, -1, ldy, ldy)
    _check_untouched(y32, M, N, label + " f32")
    e32 = _judge(label + " f32-mfma", "adm_conv_fwd", "f32", out, y32[:M, :N].reshape(B, H, W, N), ref, None, bad)
    for tile in bc.TILES:
        ys = {}
        for st in stored:
            name = "adm_conv_fwd_bf16a" if st else "adm_conv_fwd_bf16"
            lab = f"{label} {name} tile{tile}"
            y = _conv_launch(hip, name, x16 if st else x, w16, bias, res, g, tile, ldy, ldy)
            _check_untouched(y, M, N, lab)
            _judge(lab, name, "%dx%d" % bc.TILES[tile], out, y[:M, :N].reshape(B, H, W, N), ref, e32, bad)
            ys[st] = y
            RAN.add(("fwd", tile, st))
        if len(ys) == 2:
            assert torch.equal(_bits(ys[False]), _bits(ys[True])), f"{label} tile{tile}: stored-bf16 input differs from f32 input"


@pytest.mark.parametrize("g", bc.FWD, ids=bc.geom_id)
def test_forward_forms_vs_fp64(hip, g):
    """Every form x (f32 | stored-bf16 input) with bias + residual; the first geometry also with no epilogue and with ldy = ldr = N + 32."""
    B, H, W, ci, N, ks, up = g
    d, ref = bc.data(g), bc.references(g)
    x, bias = d["x"].cuda(), d["bias"].cuda()
    w_op = bc.fwd_operand(bc.r16(d["w"])).cuda()
    res = d["res"].reshape(B * H * W, N).cuda()
    bad = []
    label = bc.geom_id(g)
    _sweep_conv(hip, label, g, x, w_op, bias, res, ref["y"], "y", N, bad)
    if g == bc.FWD[0]:
        _sweep_conv(hip, label + " bare", g, x, w_op, None, None, ref["y0"], "y", N, bad)
        wide = torch.zeros(B * H * W, N + 32, device="cuda")
        wide[:, :N] = res
        _sweep_conv(hip, label + " ld+32", g, x, w_op, bias, wide, ref["y"], "y", N + 32, bad)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("g", (bc.FWD[2], bc.FWD[3], bc.FWD[6]), ids=bc.geom_id)
def test_data_gradient_forms_vs_fp64(hip, g):
    """The data gradient is the same kernel over dy with the flipped, transposed operand: every form against fp64 of (dy, w) rounded."""
    B, H, W, ci, N, ks, up = g
    d, ref = bc.data(g), bc.references(g)
    bad = []
    _sweep_conv(hip, bc.geom_id(g) + " dgrad", (B, H, W, N, ci, ks, 0), d["dy"].cuda(), bc.bwd_operand(bc.r16(d["w"])).cuda(), None, None,
                ref["dx"], "dx", ci, bad, stored=(False,))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ weight gradient
def _plan(hip, g, splits):
    B, H, W, ci, co, ks, up = g
    out = (ctypes.c_int * 4)()
    assert hip.lib().adm_conv_wgrad_bf16_plan(B * H * W, ci, co, ks, splits, out) == 0
    return tuple(out)


def _wgrad_launch(hip, sym, x, dy, g, splits, fill):
    B, H, W, ci, co, ks, up = g
    dwp = _sentinel((co, ks * ks, ci)) if fill == "nan" else torch.zeros(co, ks * ks, ci, device="cuda")
    extra = (None,) if sym == "adm_conv_wgrad_bias" else ()
    hip.call(sym, hip.ptr(x), hip.ptr(dy), hip.ptr(dwp), *extra, B, H, W, ci, ci, co, co, ks, up, splits)
    torch.cuda.synchronize()
    return dwp


def _check_wgrad(hip, g, modes, bad):
    """modes: (splits, how the buffer is filled).  Every mode on the f32-input and the stored-bf16 entry point."""
    B, H, W, ci, co, ks, up = g
    d = bc.data(g)
    ref = tuple(t.permute(0, 2, 3, 1) for t in bc.references(g)["dw"])          # [Cout][ky][kx][Cin] = the packed [Cout][taps][Cin]
    x, dy = d["x"].cuda(), d["dy"].cuda()
    x16 = x.to(torch.bfloat16)
    label = bc.geom_id(g)
    shape = (co, ks, ks, ci)
    d32 = _wgrad_launch(hip, "adm_conv_wgrad_bias", x16.to(torch.float32), bc.r16(d["dy"]).cuda(), g, 1, "nan")
    e32 = _judge(label + " f32-mfma", "adm_conv_wgrad_bias", "f32", "dw", d32.reshape(shape), ref, None, bad)
    for splits, fill in modes:
        plan = _plan(hip, g, splits)
        assert plan + (bc.is_fast(g),) == bc.WGRAD_PLANS[(g, splits)], (g, splits, plan)
        mode = "store" if plan[2] == 1 else "atomic+memset" if splits >= 0 else "atomic-prezeroed"
        outs = {}
        for st in (False, True):
            name = "adm_conv_wgrad_bf16a" if st else "adm_conv_wgrad_bf16"
            lab = f"{label} {name} splits={splits}->{plan[2]}"
            dwp = _wgrad_launch(hip, name, x16 if st else x, dy, g, splits, fill)
            _judge(lab, name, f"{plan[0]}x{plan[1]}-{'fast' if bc.is_fast(g) else 'general'}-{mode}", "dw", dwp.reshape(shape), ref, e32, bad)
            outs[st] = dwp
            RAN.add(("wgrad", plan[0], plan[1], bc.is_fast(g), st, mode))
        if plan[2] == 1:
            assert torch.equal(_bits(outs[False]), _bits(outs[True])), f"{label}: stored-bf16 x differs from f32 x"


@pytest.mark.parametrize("g", bc.WGRAD, ids=bc.geom_id)
def test_weight_gradient_forms_vs_fp64(hip, g):
    """splits = 1 into a NaN-filled buffer (every element of [Cout][taps][Cin] must be stored), f32 and stored-bf16 x bit-identical; the
    first, third and fourth geometry also at explicit splits 2 and 3 (atomics after the launcher's memset, a short last chunk)."""
    bad = []
    _check_wgrad(hip, g, [(1, "nan")] + ([(2, "nan"), (3, "nan")] if g in bc.WGRAD_SPLIT else []), bad)
    assert not bad, "\n".join(bad)


def test_weight_gradient_automatic_splits_vs_fp64(hip):
    """splits = 0 into a NaN-filled buffer (the launcher's memset must clear it) and splits = -1 into a zeroed one (the pre-zeroed
    contract of the deferred unpack): the plan query says both are atomic two-way splits."""
    bad = []
    _check_wgrad(hip, bc.WGRAD_AUTO, [(0, "nan"), (-1, "zero")], bad)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ report
def test_zz_report_worst_errors():
    """Worst e_max / e_rms (and worst ratio to the bar-B limits) per kernel, form and output; with the whole sweep run, every forward
    form on both inputs, every weight-gradient tile form, both load paths and all three split modes were executed."""
    if not WORST:
        print("no sweep ran in this session")
        return
    print("\nworst error vs fp64 of the rounded operands per kernel / form / output (e_max, e_rms, bar-B ratios max / rms):")
    for (kernel, form, out), (em, er, rm, rr) in sorted(WORST.items()):
        print(f"  {kernel:22s} {form:36s} {out:3s} {em:.3e} {er:.3e} {rm:5.2f} {rr:5.2f}")
    fwd = {r[1:] for r in RAN if r[0] == "fwd"}
    wg = {r[1:] for r in RAN if r[0] == "wgrad"}
    if len(fwd) == 6 and len({(r[0], r[1]) for r in wg}) == 4:       # the whole sweep ran
        assert {r[2] for r in wg} == {True, False} and {r[3] for r in wg} == {True, False}
        assert {r[4] for r in wg} == {"store", "atomic+memset", "atomic-prezeroed"}
