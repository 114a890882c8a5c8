"""GPU: the kernels only the SR denoiser uses (csrc/cond_ops.hip, csrc/attention_small.hip) against fp64, forward and backward.

Every row of tests/cond_cases.py is one test: the operator of adm_amd.ops_cond runs forward and backward on the row's data, twice
(every output of the second run must be bitwise the first's: the kernels combine partial sums in a fixed order, without atomics),
and every output and gradient is compared with the fp64 reference of tests/fp64ref.py, computed on the GPU from the same inputs.

Bar, per output and relative to the scale of the reference's mag (fp64ref.errors): e_max <= BAR_A, the bar of the convs, the d = 64
attention and GroupNorm (tests/test_hip_accuracy.py).  On the cases of cond_cases.FALLBACK the limit is max(BAR_A, 2 x the e_max of
the fp32 torch composition on the same data, computed in the same test on the CPU): the factor 2 of bar B, the comparator is torch,
never the kernel.  Which bar applies where:

    fallback bar    bn        M524800-C4-train-offset               (x - mean cancels 4 bits in front of 524 800-term sums)
                    bilinear  Hi128-300x3-T, Hi128-300x3-F          (the f32 source coordinate near 127 keeps 17 bits of lam)
                    fourier   wide-D16, wide-D300                   (phases of ~ 1e3 radians in fp32)
                    mha       Lq63-Lk64-D16-x6, Lq65-Lk63-D64-x6,   (logits of a few hundred: their fp32 rounding is a relative
                              Lq130-Lk130-D32-x6, packed-L65-D32-x6  error of exp())
    BAR_A           every other case of every operator: all of ws, ln, act, col2im, la and spatt, the eps / const / offset data of
                    the normalisers, the flat, uniform and one-key-dominates softmax of mha, the spread keys of la, the saturated gate

tests/test_fp64ref_cond_host.py shows on the CPU that this split is exact (plain fp32 torch is above BAR_A / 4 on the fallback cases
and at or below it on all others) and that the bar rejects an ignored or wrong eps, the wrong variance divisor, the wrong
align_corners, a missing 1 / N, a softmax over the wrong axis, a scale applied twice, an lse without the running maximum and a
softsign derivative without its square.

Dropout: the mask is recovered from y (a dropped element is 0 where the undropped fp64 output is not) and the backward must have used
the same one.  The direct-gradient sinks (accumulate = 1 of adm_ws_bwd, adm_lnc_bwd, adm_bn_bwd) are called through the C ABI on a
buffer pre-filled with known values: the result is prefill + gradient, at the same bar against mag + |prefill|.
"""
import math

import pytest
import torch

import cond_cases as cc
import fp64ref
from test_hip_accuracy import BAR_A

pytestmark = pytest.mark.gpu

WORST = {}          # (kernel, bar, output) -> [e_max, e_rms, case of e_max]
ACT_CODE = {"id": 0, "relu": 1, "gelu": 2}


@pytest.fixture(scope="module")
def oc():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip, ops_cond
    hip.lib()        # raises if the HIP library is missing: no fallback
    return ops_cond


def _dev(t, grad=False):
    return t.cuda().contiguous().requires_grad_(grad)


def _kernel(op, case):
    if op == "bn":
        return "batch_norm " + ("train" if case[4] else "eval")
    if op == "mha":
        return f"mha D{case[5]}" + (" packed" if case[8] else "")
    if op == "bilinear":
        return "bilinear_into" if case[8] else "bilinear"
    return {"ws": "weight_standardize", "ln": "layer_norm_c", "act": "act " + str(case[2]), "fourier": "fourier_features",
            "col2im": "col2im", "la": "linear_attention", "spatt": "spatial_att_gate (any size)"}[op]


def _run(oc, op, case, d):
    """One forward and backward of a case on the GPU: the outputs under the names of cond_cases.reference()."""
    from adm_amd import hip
    if op == "ws":
        w = _dev(d["w"], True)
        y = oc.weight_standardize(w)
        y.backward(_dev(d["dy"]))
        return dict(y=y.detach(), dw=w.grad)
    if op == "ln":
        x, g = _dev(d["x"], True), _dev(d["g"], True)
        y = oc.layer_norm_c(x, g)
        y.backward(_dev(d["dy"]))
        return dict(y=y.detach(), dx=x.grad, dg=g.grad)
    if op == "bn":
        C, training = case[2], case[4]
        bn = torch.nn.BatchNorm2d(C, momentum=cc.BN_MOMENTUM, eps=cc.BN_EPS).cuda()
        with torch.no_grad():
            for p, n in ((bn.weight, "gamma"), (bn.bias, "beta"), (bn.running_mean, "run_mean"), (bn.running_var, "run_var")):
                p.copy_(d[n])
        x = _dev(d["x"], True)
        y = oc.batch_norm(x, bn, training)
        y.backward(_dev(d["dy"]))
        assert int(bn.num_batches_tracked) == int(training)
        return dict(y=y.detach(), running_mean=bn.running_mean.detach(), running_var=bn.running_var.detach(), dx=x.grad,
                    dgamma=bn.weight.grad, dbeta=bn.bias.grad)
    if op == "bilinear":
        _, B, Hi, Wi, Ho, Wo, C, align, into = case
        x = _dev(d["x"], True)
        if into is None:
            y = oc.bilinear(x, Ho, Wo, align)
            y.backward(_dev(d["dy"]))
            return dict(y=y.detach(), dx=x.grad)
        coff = into[0]
        buf = _dev(d["buf"]).clone()
        out = oc.bilinear_into(x, buf, coff, align)
        assert out.data_ptr() == buf.data_ptr()
        for sl in (slice(0, coff), slice(coff + C, None)):                   # the neighbouring channels keep their values
            assert torch.equal(out.detach()[..., sl], _dev(d["buf"])[..., sl]), (case[0], "wrote outside its channels")
        out.backward(_dev(d["dbuf"]))
        return dict(y=out.detach()[..., coff:coff + C], dx=x.grad)
    if op == "act":
        _, shape, kind, p = case
        x = _dev(d["x"], True)
        y = oc._Act.apply(x, ACT_CODE[kind], float(p), cc.DROP_SEED if p > 0 else 0)     # (a fixed seed: both runs drop the same elements)
        y.backward(_dev(d["dy"]))
        return dict(y=y.detach(), dx=x.grad)
    if op == "fourier":
        return dict(y=oc.fourier_features(_dev(d["x"]), _dev(d["W"])))
    if op == "col2im":
        _, B, Hin, Win, C, ks, stride, pad = case
        col = _dev(d["col"])
        dx = torch.full((B, Hin, Win, C), float("nan"), device="cuda")
        hip.call("adm_col2im", hip.ptr(col), hip.ptr(dx), B, Hin, Win, col.shape[1], col.shape[2], C, ks, stride, pad)
        return dict(dx=dx)
    if op == "mha":
        heads, scale, packed = case[4], case[6], case[8]
        if packed:
            qkv = _dev(d["qkv"], True)
            o = oc.self_attention_packed(qkv, heads, scale)
            o.backward(_dev(d["dout"]))
            return dict(out=o.detach(), dqkv=qkv.grad)
        q, k, v = (_dev(d[n], True) for n in "qkv")
        o = oc.mha(q, k, v, heads, scale)
        o.backward(_dev(d["dout"]))
        return dict(out=o.detach(), dq=q.grad, dk=k.grad, dv=v.grad)
    if op == "la":
        qkv = _dev(d["qkv"], True)
        o = oc.linear_attention(qkv)
        o.backward(_dev(d["dout"]))
        return dict(out=o.detach(), dqkv=qkv.grad)
    if op == "spatt":
        att, qk, h, xres = (_dev(d[n], True) for n in ("att", "qk", "h", "xres"))
        y = oc._SpatialAttBig.apply(att, qk, h, xres)                        # (ops_cond.spatial_att_gate sends <= 64 pixels elsewhere)
        y.backward(_dev(d["dy"]))
        assert torch.equal(xres.grad, _dev(d["dy"]))
        return dict(y=y.detach(), dh=h.grad, datt=att.grad, dqk=qk.grad)
    raise KeyError(op)


def _note(kernel, bar, out, e, name):
    w = WORST.setdefault((kernel, bar, out), [0.0, 0.0, ""])
    if e[0] >= w[0]:
        w[0], w[2] = e[0], name
    w[1] = max(w[1], e[1])


def _compare(op, case, got, ref, e32):
    """Every output of ref against its bar; e32 = fp32 torch's e_max per output (fallback cases) or None.  Everything is printed
    before anything is asserted."""
    lines, bad = [], []
    bar = "BAR_A" if e32 is None else "fallback"
    for n, (r, mag) in ref.items():
        assert got[n].shape == r.shape, (case[0], n, got[n].shape, r.shape)
        e = fp64ref.errors(got[n], r, mag)
        _note(_kernel(op, case), bar, n, e, case[0])
        lim = BAR_A if e32 is None else max(BAR_A, 2.0 * e32[n])
        lines.append(f"{n} {e[0]:.2e}/{e[1]:.2e}" + ("" if e32 is None else f" (fp32 torch {e32[n]:.2e}, limit {lim:.2e})"))
        if not (e[0] <= lim and bool(torch.isfinite(got[n]).all())):
            bad.append((n, e, lim))
    print(f"  {op} {case[0]} [{bar}] e_max/e_rms: " + ", ".join(lines))
    assert not bad, (op, case[0], bad)


def _case_test(oc, op, case):
    d = cc.make(op, case)
    got = _run(oc, op, case, d)
    again = _run(oc, op, case, d)
    keep = None
    if op == "act" and case[3] > 0:
        p = case[3]
        y0 = fp64ref.act(d["x"].cuda(), case[2])["y"][0]                      # undropped
        kept = fp64ref.recover_keep(got["y"], y0)
        vis = y0 != 0                                                        # where a drop can be seen
        frac = 1.0 - float(kept[vis].mean())
        assert abs(frac - p) <= 6.0 * math.sqrt(p * (1 - p) / int(vis.sum())), (case[0], frac)
        keep = kept / (1.0 - p)
    ref = cc.reference(op, case, d, device="cuda", **({} if keep is None else {"keep": keep}))
    assert set(ref) == set(got), (sorted(ref), sorted(got))
    e32 = None
    if cc.is_fallback(op, case):
        t32 = cc.torch32(op, case, d, **({} if keep is None else {"keep": keep}))
        e32 = {n: fp64ref.errors(t32[n], *ref[n])[0] for n in ref}
    _compare(op, case, got, ref, e32)
    for n in got:
        assert torch.equal(got[n], again[n]), (op, case[0], n, "the second run differs from the first")
    return d, got


@pytest.mark.parametrize("case", cc.CASES["ws"], ids=cc.ids("ws"))
def test_weight_standardize(oc, case):
    d, got = _case_test(oc, "ws", case)
    if case[4] == "const":                   # a constant row: mean exact, every deviation 0, rstd = eps^-1/2 finite
        assert int(torch.count_nonzero(got["y"][0])) == 0 and bool(torch.isfinite(got["dw"][0]).all())


@pytest.mark.parametrize("case", cc.CASES["ln"], ids=cc.ids("ln"))
def test_layer_norm_c(oc, case):
    d, got = _case_test(oc, "ln", case)
    if case[3] == "const":                   # (C is a power of two in these rows: sum / C is exact in any order)
        assert int(torch.count_nonzero(got["y"][0, 0])) == 0 and bool(torch.isfinite(got["dx"][0, 0]).all())


@pytest.mark.parametrize("case", cc.CASES["bn"], ids=cc.ids("bn"))
def test_batch_norm(oc, case):
    d, got = _case_test(oc, "bn", case)
    if case[3] == "const":                   # a constant channel: xhat = 0, y = beta at every pixel
        y0 = got["y"][..., 0]
        assert bool(torch.isfinite(y0).all()) and torch.equal(y0, d["beta"][0].cuda().expand_as(y0))
        assert bool(torch.isfinite(got["dx"][..., 0]).all())


@pytest.mark.parametrize("case", cc.CASES["bilinear"], ids=cc.ids("bilinear"))
def test_bilinear(oc, case):
    _case_test(oc, "bilinear", case)


@pytest.mark.parametrize("case", cc.CASES["act"], ids=cc.ids("act"))
def test_activation_dropout(oc, case):
    _case_test(oc, "act", case)


@pytest.mark.parametrize("case", cc.CASES["fourier"], ids=cc.ids("fourier"))
def test_fourier_features(oc, case):
    _case_test(oc, "fourier", case)


@pytest.mark.parametrize("case", cc.CASES["col2im"], ids=cc.ids("col2im"))
def test_col2im(oc, case):
    _case_test(oc, "col2im", case)


@pytest.mark.parametrize("case", cc.CASES["mha"], ids=cc.ids("mha"))
def test_mha(oc, case):
    d, got = _case_test(oc, "mha", case)
    if case[7] == "equal":                   # all keys equal: every weight is 1 / Lk, whatever the query
        v = d["v"].cuda().double().mean(dim=1, keepdim=True).expand_as(got["out"])
        assert float((got["out"].double() - v).abs().max()) <= BAR_A * float(d["v"].abs().mean())


@pytest.mark.parametrize("case", cc.CASES["la"], ids=cc.ids("la"))
def test_linear_attention(oc, case):
    _case_test(oc, "la", case)


@pytest.mark.parametrize("case", cc.CASES["spatt"], ids=cc.ids("spatt"))
def test_spatial_att_gate(oc, case):
    d, got = _case_test(oc, "spatt", case)
    assert int(torch.count_nonzero(got["datt"][..., 1:])) == 0               # only channel 0 is the map


# ------------------------------------------------------------------------------------------------ the direct-gradient sinks
def _prefill(shape, tag):
    gen = torch.Generator().manual_seed(sum(tag.encode()))
    return (torch.rand(*shape, generator=gen) * 2 - 1) * 3.0


def _check_accumulated(name, out, got, prefill, ref):
    r, mag = ref
    e = fp64ref.errors(got, r + prefill.cuda().double().reshape(r.shape), mag + prefill.cuda().double().abs().reshape(r.shape))
    _note(name + " accumulate", "BAR_A", out, e, "")
    print(f"  {name} accumulate = 1: {out} {e[0]:.2e}/{e[1]:.2e}")
    assert e[0] <= BAR_A, (name, out, e)


def test_weight_standardize_accumulates(oc):
    from adm_amd import hip
    case = cc.by_id("ws", "K1152-eps")
    d = cc.make("ws", case)
    ref = cc.reference("ws", case, d, device="cuda")
    w, dy = _dev(d["w"]), _dev(d["dy"])
    O, K = w.shape[0], w[0].numel()
    wn, stats = torch.empty_like(w), torch.empty(O, 2, device="cuda")
    pre = _prefill(tuple(w.shape), "ws")
    dw = _dev(pre).clone()
    hip.call("adm_ws_fwd", hip.ptr(w), hip.ptr(wn), hip.ptr(stats), O, K, cc.WS_EPS)
    hip.call("adm_ws_bwd", hip.ptr(w), hip.ptr(stats), hip.ptr(dy), hip.ptr(dw), O, K, 1)
    _check_accumulated("weight_standardize", "dw", dw, pre, ref["dw"])


def test_layer_norm_c_accumulates(oc):
    from adm_amd import hip
    case = cc.by_id("ln", "M257-C384-eps")                                    # two workgroups of partials
    d = cc.make("ln", case)
    ref = cc.reference("ln", case, d, device="cuda")
    x, dy, g = _dev(d["x"]), _dev(d["dy"]), _dev(d["g"])
    M, C = case[1], case[2]
    blocks = hip.lib().adm_lnc_blocks(M)
    assert blocks == 2
    part = torch.empty(blocks * C, device="cuda", dtype=torch.float64)
    pre = _prefill((C,), "ln")
    dx, dg = torch.empty_like(x), _dev(pre).clone()
    hip.call("adm_lnc_bwd", hip.ptr(x), hip.ptr(dy), hip.ptr(g), hip.ptr(dx), hip.ptr(dg), hip.ptr(part), M, C, cc.LN_EPS, 1)
    _check_accumulated("layer_norm_c", "dg", dg, pre, ref["dg"])
    e = fp64ref.errors(dx, *ref["dx"])
    assert e[0] <= BAR_A, e


def test_batch_norm_accumulates(oc):
    from adm_amd import hip
    case = cc.by_id("bn", "M1025-C12-train-const")                            # three workgroups of partials
    d = cc.make("bn", case)
    ref = cc.reference("bn", case, d, device="cuda")
    x, dy, gamma, beta = (_dev(d[n]) for n in ("x", "dy", "gamma", "beta"))
    rm, rv = _dev(d["run_mean"]).clone(), _dev(d["run_var"]).clone()
    M, C = case[1], case[2]
    blocks = hip.lib().adm_bn_blocks(M)
    assert blocks == 3
    part = torch.empty(blocks * 2 * C, device="cuda", dtype=torch.float64)
    mr, sums, y, dx = torch.empty(C, 2, device="cuda"), torch.empty(2 * C, device="cuda"), torch.empty_like(x), torch.empty_like(x)
    hip.call("adm_bn_fwd", hip.ptr(x), hip.ptr(gamma), hip.ptr(beta), hip.ptr(rm), hip.ptr(rv), hip.ptr(mr), hip.ptr(y), hip.ptr(part), M, C,
             cc.BN_EPS, cc.BN_MOMENTUM, 1)
    pg, pb = _prefill((C,), "bn.g"), _prefill((C,), "bn.b")
    dg, db = _dev(pg).clone(), _dev(pb).clone()
    hip.call("adm_bn_bwd", hip.ptr(x), hip.ptr(dy), hip.ptr(mr), hip.ptr(gamma), hip.ptr(dx), hip.ptr(dg), hip.ptr(db), hip.ptr(part),
             hip.ptr(sums), M, C, 1, 1)
    _check_accumulated("batch_norm", "dgamma", dg, pg, ref["dgamma"])
    _check_accumulated("batch_norm", "dbeta", db, pb, ref["dbeta"])
    e = fp64ref.errors(dx, *ref["dx"])
    assert e[0] <= BAR_A, e


def test_zz_report_worst_cond_errors():
    """Worst e_max / e_rms against fp64 per kernel and output (the table of DESIGN.md)."""
    if not WORST:
        pytest.skip("no case ran in this session")
    print("\nSR denoiser kernels: worst error vs fp64 per kernel / bar / output (e_max, e_rms, case of the worst e_max):")
    for (kernel, bar, out), (em, er, name) in sorted(WORST.items()):
        print(f"  {kernel:32s} {bar:9s} {out:13s} {em:.3e} {er:.3e}  {name}")
