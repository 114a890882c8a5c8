"""GPU: every compiled form of the UNet attention kernels (csrc/attention.hip, csrc/attention_h3.hip) against fp64.

tests/attn_cases.py holds the table: a geometry per sequence length, three kinds of data and, per case, the modes it runs in --
which forward and which backward entry point ops.attention takes.  tests/test_attn_cases_host.py shows on the CPU that the table
reaches every form adm_attn_form can answer up to L = 1024 and that plain fp32 torch is inside the limits used here.

Per case and mode: out and dqkv against fp64ref.attention, finite everywhere, exactly the expected symbols launched (the ops.call
recorder of tests/test_hip_accuracy.py), and the bound vector of dqkv equal to max |dqkv|.

Limits, relative to the same products on |operands| (fp64ref.errors):
  hashed data          bar A (e_max <= 1e-5) in every mode; bar B (fp64ref.bar_b) for the modes with the fp16-format forward, against
                       the f32 mode on the same data
  peaked, stair data   max(bar A, 2 x e_max of the fp32 torch restatement on the same data) = attn_cases.limit

Then: no write outside the outputs at the partial-tile lengths, (batch, head) problems independent of their neighbours to the bit,
the lengths the kernels refuse, and the worst errors per (symbol, form, mode, output).
"""
import ctypes

import pytest
import torch

import attn_cases as ac
import fp64ref
from test_hip_accuracy import Recorder

pytestmark = pytest.mark.gpu

WORST = {}        # (symbol, form, mode, output) -> [e_max, e_rms]
SENTINEL = -12345.5
GUARD = 1024      # floats: 4 KB on either side of an output


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip, ops as _ops
    hip.lib()        # raises if the HIP library is missing: no fallback
    return _ops


_DEV = {}


def _dev(case):
    """The case's data on the GPU and its fp64 reference computed there, once per case."""
    if case not in _DEV:
        qkv, dout = (t.cuda() for t in ac.data(case))
        _DEV[case] = (qkv, dout, fp64ref.attention(qkv, case.geom[3], dout))
    return _DEV[case]


def _run(ops, mp, qkv, dout, heads, mode, bound_qkv=None, bound_dout=None, slot=None):
    """ops.attention forward and backward in a mode of attn_cases.MODES, brought about with the module's own switches.  The bounds of
    qkv and dout default to their exact maxima.  Returns (out, dqkv, (tensor, vector) of the bound the backward registered or None)."""
    for name in ("ATTN_H3", "ATTN_H3_BWD", "BF16X6", "H3_GEMM"):
        mp.setattr(ops, name, True)
    mp.setattr(ops, "COMPUTE", "f32")
    mp.setattr(ops, "FP16X3", mode != "f32")
    gvec = None
    if mode == "h3":
        gvec = ops.amax_vector(dout) if bound_dout is None else bound_dout
    mp.setattr(ops, "_get_amax", lambda t: gvec)
    registered = []
    mp.setattr(ops, "_reg_amax", lambda t, v: registered.append((t, v)))
    if slot is not None:
        mp.setattr(ops, "_amax_slot", lambda like: slot)
    qd = qkv.clone().requires_grad_(True)
    if mode in ("h3", "h3-fwd"):
        qd._adm_amax = ops.amax_vector(qd) if bound_qkv is None else bound_qkv
    a = ops.attention(qd, heads)
    a.backward(dout)
    torch.cuda.synchronize()
    assert len(registered) == 1
    t, v = registered[0]
    assert torch.equal(t, qd.grad)
    return a.detach(), qd.grad, (None if v is None else (t, v))


def _launched(rec):
    return sorted(k for ks in rec.launches.values() for k in ks)


def _note(sym, L, mode, out, e):
    w = WORST.setdefault((sym, ac.form_label(ac.FAMILY[sym], L), mode, out), [0.0, 0.0])
    w[0], w[1] = max(w[0], e[0]), max(w[1], e[1])


@pytest.mark.parametrize("case", ac.CASES, ids=ac.case_id)
def test_attention_forms_vs_fp64(ops, monkeypatch, case):
    """Every mode of the case: launches, finiteness, out and dqkv against fp64 within the case's limits, the bound of dqkv."""
    B, H, W, heads = case.geom
    L = H * W
    qkv, dout, ref = _dev(case)
    rec = Recorder(monkeypatch)
    errs, bad = {}, []
    for mode in case.modes:              # "f32" first: bar B compares with it
        rec.launches = {}
        a, dqkv, reg = _run(ops, monkeypatch, qkv, dout, heads, mode)
        fwd, bwd = ac.MODES[mode]
        assert _launched(rec) == sorted([(fwd, (B, L, heads), "pppp" if fwd.endswith("h3") else "ppp"),
                                         (bwd, (B, L, heads), {"adm_attn_bwd": "pppppp", "adm_attn_bwd_amax": "ppppppp",
                                                               "adm_attn_bwd_h3": "ppppppppp"}[bwd])]), (mode, _launched(rec))
        if mode == "f32":
            assert reg is None
        else:                            # the kernels take the maximum of the very values they store
            vec = reg[1]
            assert float(vec.max()) == float(dqkv.abs().max()) and float(vec.min()) >= 0.0, (mode, float(vec.max()), float(dqkv.abs().max()))
        for out, t, sym in (("out", a, fwd), ("dqkv", dqkv, bwd)):
            assert bool(torch.isfinite(t).all()), (mode, out)
            e = fp64ref.errors(t, *ref[out])
            errs[(mode, out)] = e
            _note(sym, L, mode, out, e)
            lim = ac.limit(case, out)
            print(f"{ac.case_id(case)} {mode:8s} {out:4s} e_max {e[0]:.3e} e_rms {e[1]:.3e} limit {lim:.1e}")
            if e[0] > lim:
                bad.append(f"limit: {mode} {out} e_max {e[0]:.3e} > {lim:.3e}")
            if case.kind == "hashed" and mode in ("h3", "h3-fwd"):
                ok, rm, rr = fp64ref.bar_b(e, errs[("f32", out)])
                if not ok:
                    bad.append(f"bar B: {mode} {out} e {e[0]:.3e}/{e[1]:.3e} vs f32 {errs[('f32', out)][0]:.3e}/"
                               f"{errs[('f32', out)][1]:.3e} (ratios {rm:.2f}, {rr:.2f})")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mode", ["f32+amax", "h3", "h3-fwd"])
def test_bound_vector_is_raised_never_overwritten(ops, monkeypatch, mode):
    """A vector that already holds more than max |dqkv| in every slot comes back as it was: the kernels raise with atomicMax."""
    case = next(c for c in ac.CASES if c.kind == "hashed" and ac.seq_len(c) == 64)
    qkv, dout, _ = _dev(case)
    pre = torch.full((ops.AMAX_FLOATS,), 1000.0, device="cuda")
    _, dqkv, reg = _run(ops, monkeypatch, qkv, dout, case.geom[3], mode, slot=pre)
    assert reg[1] is pre and 0.0 < float(dqkv.abs().max()) < 1000.0
    assert torch.equal(pre, torch.full_like(pre, 1000.0))


@pytest.mark.parametrize("mode", ["f32+amax", "h3", "h3-fwd"])
def test_bound_vector_covers_each_third(ops, monkeypatch, mode):
    """Data on which dq, dk and dv in turn hold max |dqkv| (attn_cases.BOUND_SCALES): the bound equals that maximum each time."""
    for i, which in enumerate(("dq", "dk", "dv")):
        qkv, dout, heads = ac.bound_data(which)
        _, dqkv, reg = _run(ops, monkeypatch, qkv.cuda(), dout.cuda(), heads, mode)
        m = ac.third_maxima(dqkv, heads)
        assert m[i] == max(m) and float(reg[1].max()) == m[i], (which, m, float(reg[1].max()))


def _guarded(n):
    """(whole buffer, payload view of n floats) with GUARD sentinel floats on either side."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


@pytest.mark.parametrize("L,family", [(1, "f32"), (9, "f32"), (25, "f32"), (32, "h3")])
def test_no_stray_writes(ops, monkeypatch, L, family):
    """The entry points called directly on outputs with a 4 KB sentinel guard on either side: the guards stay, and the payload is what
    ops.attention returns (the partial-tile lengths of the f32 family, where rows and keys past L are guarded; the smallest h3 form)."""
    from adm_amd import hip
    case = next(c for c in ac.CASES if c.kind == "hashed" and ac.seq_len(c) == L)
    B, H, W, heads = case.geom
    qkv, dout, _ = _dev(case)
    n_out, n_row = B * L * heads * 64, B * heads * L
    p = hip.ptr
    runs = [("adm_attn_bwd", "f32"), ("adm_attn_bwd_amax", "f32+amax")] if family == "f32" else [("adm_attn_bwd_h3", "h3")]
    aq, ag = ops.amax_vector(qkv), ops.amax_vector(dout)
    for bwd, mode in runs:
        want_out, want_dqkv, reg = _run(ops, monkeypatch, qkv, dout, heads, mode)
        bufs = {n: _guarded(k) for n, k in (("out", n_out), ("lse", n_row), ("delta", n_row), ("dqkv", qkv.numel()))}
        out, lse, delta, dqkv = (bufs[n][1] for n in ("out", "lse", "delta", "dqkv"))
        slot = torch.zeros(ops.AMAX_FLOATS, device="cuda")
        if family == "f32":
            hip.call("adm_attn_fwd", p(qkv), p(out), p(lse), B, L, heads)
            if bwd == "adm_attn_bwd":
                hip.call(bwd, p(qkv), p(out), p(dout), p(lse), p(dqkv), p(delta), B, L, heads)
            else:
                hip.call(bwd, p(qkv), p(out), p(dout), p(lse), p(dqkv), p(delta), p(slot), B, L, heads)
        else:
            hip.call("adm_attn_fwd_h3", p(qkv), p(out), p(lse), p(aq), B, L, heads)
            hip.call(bwd, p(qkv), p(out), p(dout), p(lse), p(dqkv), p(delta), p(aq), p(ag), p(slot), B, L, heads)
        torch.cuda.synchronize()
        for n, (buf, _) in bufs.items():
            assert _guards_intact(buf), (bwd, n)
        assert torch.equal(out.reshape(want_out.shape), want_out) and torch.equal(dqkv.reshape(want_dqkv.shape), want_dqkv), bwd
        assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(delta).all())
        if reg is not None:
            assert float(slot.max()) == float(reg[1].max())


@pytest.mark.parametrize("L,mode", [(25, "f32+amax"), (288, "f32+amax"), (64, "h3"), (512, "h3")])
def test_batch_and_head_independence(ops, monkeypatch, L, mode):
    """A (B = 2, heads = 3) problem, and each of its (b, head) cut out and run as B = 1, heads = 1 with the same bounds: the same bits."""
    H, W = ac.GEOM[L][1:3]
    from oracle import fill
    qkv = fill.hash_tensor((2, H, W, 3 * 192), f"attnforms.indep.qkv.{L}", 1.0).cuda()
    dout = fill.hash_tensor((2, H, W, 3 * 64), f"attnforms.indep.g.{L}", 1.0).cuda()
    aq, ag = ops.amax_vector(qkv), ops.amax_vector(dout)
    out, dqkv, _ = _run(ops, monkeypatch, qkv, dout, 3, mode, aq, ag)
    for b in range(2):
        for h in range(3):
            o1, d1, _ = _run(ops, monkeypatch, qkv[b:b + 1, :, :, h * 192:(h + 1) * 192].contiguous(),
                             dout[b:b + 1, :, :, h * 64:(h + 1) * 64].contiguous(), 1, mode, aq, ag)
            assert torch.equal(o1, out[b:b + 1, :, :, h * 64:(h + 1) * 64]), (b, h)
            assert torch.equal(d1, dqkv[b:b + 1, :, :, h * 192:(h + 1) * 192]), (b, h)


def test_refused_lengths(ops, monkeypatch):
    """ADM_EINVAL without a launch (the output keeps its sentinel) from adm_attn_fwd at L = 33, 100, 144 and from adm_attn_fwd_h3 at
    L = 96, 320; ops.attention with a bound at L = 96 and 320 takes the f32 kernels."""
    from adm_amd import hip
    from oracle import fill
    lib, p = hip.lib(), hip.ptr
    for sym, L in [("adm_attn_fwd", 33), ("adm_attn_fwd", 100), ("adm_attn_fwd", 144), ("adm_attn_fwd_h3", 96), ("adm_attn_fwd_h3", 320)]:
        qkv = torch.zeros(1, L, 192, device="cuda")
        out, lse = torch.full((L * 64,), SENTINEL, device="cuda"), torch.full((L,), SENTINEL, device="cuda")
        bound = ops.amax_vector(qkv + 1.0)
        args = (p(qkv), p(out), p(lse)) + ((p(bound),) if sym.endswith("h3") else ()) + (1, L, 1, hip.stream())
        assert getattr(lib, sym)(*args) == -22, (sym, L)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((lse == SENTINEL).all()), (sym, L)
    rec = Recorder(monkeypatch)
    for H, W in ((8, 12), (16, 20)):
        L = H * W
        qkv = fill.hash_tensor((1, H, W, 2 * 192), f"attnforms.refused.qkv.{L}", 1.0).cuda()
        dout = fill.hash_tensor((1, H, W, 2 * 64), f"attnforms.refused.g.{L}", 1.0).cuda()
        ref = fp64ref.attention(qkv, 2, dout)
        rec.launches = {}
        a, dqkv, reg = _run(ops, monkeypatch, qkv, dout, 2, "h3")          # bounds on qkv and dout: h3 wherever it can run
        assert [k[0] for k in _launched(rec)] == ["adm_attn_bwd_amax", "adm_attn_fwd"], _launched(rec)
        assert float(reg[1].max()) == float(dqkv.abs().max())
        for out, t in (("out", a), ("dqkv", dqkv)):
            e = fp64ref.errors(t, *ref[out])
            assert e[0] <= ac.BAR_A, (L, out, e)


def test_zz_report_worst_errors():
    """Worst e_max / e_rms per (symbol, form, mode, output) over the sweep."""
    if not WORST:
        pytest.skip("no sweep ran in this session")
    print("\nworst error vs fp64 per symbol / form / mode / output (e_max, e_rms):")
    for (sym, form, mode, out), (em, er) in sorted(WORST.items()):
        print(f"  {sym:18s} {form:22s} {mode:9s} {out:4s} {em:.3e} {er:.3e}")
