"""GPU: the schedule, loss, sampler, optimiser and layout kernels of adm_amd/csrc/elementwise.hip against the float64 references of
tests/elementwise_ref.py, at ragged sizes (B = 3 with distinct per-sample scalars, totals that are no multiple of 4, 64 or 256) and at
sizes whose threads make a second trip of the grid-stride loop (the grid is capped at 8192 workgroups of 256).

Bars, per output and relative to the reference's mag (fp64ref.errors):
  data movement (scale 1, coefficient 1, ema_decay 0, pad channels)      torch.equal
  fp32 kernels                                                           fp64ref.bar_b(e, e32), e32 = fp32 torch on the same data by the
                                                                         same helper, and e_max <= BAR_A (tests/test_elementwise_ref_host.py
                                                                         shows e32 <= BAR_A / 4 on all data used here: the ceiling never decides)
  fp64 sampler state                                                     e_max <= 2 k 2^-53, k = the formula's rounded operations
                                                                         (counted in elementwise_ref.py); no fp32 baseline
  bound vectors                                                          max over the slots == max |y| bitwise; all-zero output: untouched
The one-workgroup loss path and sumsq with partials must repeat bitwise; the chunked loss sums and sumsq without partials (float /
double atomics) are on bar B only.  Arguments production reaches go through ops / optim; combinations only the header documents go
through hip.call.  The references run in torch on the GPU (float64 / float32 elementwise kernels and sums of torch, none of this project).
The loss cases have 24 samples (elementwise_ref.LOSS_B says why: e_rms of three sums is the rounding of one f32 value); every other
ragged case has B = 3.  profiles/elementwise_errors.md holds the measured errors and what these cases found in the kernels.
"""
import os
import types

import pytest
import torch

import elementwise_ref as er
import fp64ref
from test_hip_accuracy import BAR_A

pytestmark = pytest.mark.gpu

WORST = {}          # (kernel, output) -> [e_max, e_rms, ratio to the limit, which bar]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip, ops as _ops
    hip.lib()        # raises if the HIP library is missing: no fallback
    return _ops


def dev(t):
    return None if t is None else t.cuda()


def _note(kernel, out, e, ratio, bar):
    w = WORST.setdefault((kernel, out), [0.0, 0.0, 0.0, bar])
    w[0], w[1], w[2] = max(w[0], e[0]), max(w[1], e[1]), max(w[2], ratio)


def check(kernel, got, ref, ref32, where=""):
    """every output of `ref` ({name: (value, mag)}) on bar B against the fp32 baseline `ref32`"""
    for n, (r, mag) in ref.items():
        g = got[n]
        assert g.shape == r.shape, (kernel, n, g.shape, r.shape)
        assert bool(torch.isfinite(g).all()), (kernel, n, where)
        e = fp64ref.errors(g, r, mag)
        e32 = fp64ref.errors(ref32[n][0], r, mag)
        ok, r_max, r_rms = fp64ref.bar_b(e, e32)
        _note(kernel, n, e, max(r_max, r_rms), "B")
        print(f"  {kernel} {where} {n}: e_max {e[0]:.2e} e_rms {e[1]:.2e} (fp32 torch {e32[0]:.2e} / {e32[1]:.2e}) ratio {r_max:.2f} / {r_rms:.2f}")
        assert ok and e[0] <= BAR_A, (kernel, where, n, e, e32, r_max, r_rms)


def check64(kernel, got, ref, k, where=""):
    """the fp64 sampler state: e_max <= 2 k 2^-53 of mag"""
    r, mag = ref["x"]
    assert got.dtype == torch.float64 and bool(torch.isfinite(got).all()), (kernel, where)
    e = fp64ref.errors(got, r, mag)
    lim = 2 * k * 2.0 ** -53
    _note(kernel, "x", e, e[0] / lim, f"2 k 2^-53, k = {k}")
    assert e[0] <= lim, (kernel, where, e, lim)


def exact(kernel, out, got, ref):
    assert torch.equal(got, ref.to(got.dtype)), (kernel, out, float((got.double() - ref.double()).abs().max()))
    _note(kernel, out, (0.0, 0.0), 0.0, "equal")


def slot(fill=0.0):
    from adm_amd import ops as _ops
    return torch.full((_ops.AMAX_FLOATS,), fill, device="cuda", dtype=torch.float32)


def check_bound(kernel, s, y):
    """the bound vector holds max |y| bitwise (its maximum over the slots: ops.amax_vector's reading)"""
    assert float(s.max()) == float(y.abs().max()) and float(s.min()) >= 0.0, (kernel, float(s.max()), float(y.abs().max()))


# ------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("n", [er.RAGGED_N, er.WRAP_B3])
@pytest.mark.parametrize("schedule", [0, 1])
def test_q_sample(ops, schedule, n):
    x0, noise = dev(er.data((3, n), "q.x0", 1.0)), dev(er.data((3, n), "q.noise", 1.7))
    for t in er.t_triples() if n == er.RAGGED_N else er.t_triples()[:1]:
        t = dev(t)
        got = ops.q_sample(x0, noise, t, schedule)
        check("q_sample", {"xt": got}, er.q_sample(x0, noise, t, schedule), er.q_sample(x0, noise, t, schedule, torch.float32),
              f"schedule {schedule} n {n} t {t.tolist()}")


# ------------------------------------------------------------------------------------------------ loss
def _loss_args(n, schedule):
    return {k: dev(v) for k, v in er.loss_data(n, schedule).items()}


@pytest.mark.parametrize("n", er.LOSS_NS)
@pytest.mark.parametrize("schedule", [0, 1])
def test_ddm_loss(ops, schedule, n):
    from adm_amd import hip
    d = _loss_args(n, schedule)
    w = d["w"][:, :2].contiguous()
    B = er.LOSS_B
    gs = er.f32(1.0 / B)
    ref = er.ddm_loss(d["c"], d["e"], d["x0"], d["noise"], w, gs)
    ref32 = er.ddm_loss(d["c"], d["e"], d["x0"], d["noise"], w, gs, torch.float32)
    c, e = d["c"].clone().requires_grad_(True), d["e"].clone().requires_grad_(True)
    loss, per = ops.ddm_loss(c, e, d["x0"], d["noise"], w)
    loss.backward()
    check("ddm_loss", {"per": per, "d_c": c.grad, "d_n": e.grad}, ref, ref32, f"schedule {schedule} n {n}")
    # gradients not requested (d_c = d_n = NULL), twice
    runs = []
    for _ in range(2):
        p = torch.full((B,), 7.0, device="cuda", dtype=torch.float64)          # (fp64 sums; the entry point zeroes them)
        hip.call("adm_ddm_loss", hip.ptr(d["c"]), hip.ptr(d["e"]), hip.ptr(d["x0"]), hip.ptr(d["noise"]), hip.ptr(w), hip.ptr(p), None, None,
                 gs, B, n)
        runs.append(p.float())
    check("ddm_loss", {"per": runs[0]}, {"per": ref["per"]}, ref32, f"no gradients, schedule {schedule} n {n}")
    if n <= 65536:          # one workgroup per sample: reproducible (above: up to 64 chunks summed with atomics, bar B only)
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], per)


@pytest.mark.parametrize("n", er.LOSS_NS)
@pytest.mark.parametrize("use_l1", [False, True])
@pytest.mark.parametrize("schedule", [0, 1])
def test_ddm_loss_latent(ops, schedule, use_l1, n):
    from adm_amd import hip
    d = _loss_args(n, schedule)
    B = er.LOSS_B
    gs = er.f32(1.0 / B)
    a = (d["c"], d["e"], d["x0"], d["noise"], d["xt"], d["t"], d["w"], gs, schedule, use_l1)
    ref, ref32 = er.ddm_loss_latent(*a), er.ddm_loss_latent(*a, torch.float32)
    c, e = d["c"].clone().requires_grad_(True), d["e"].clone().requires_grad_(True)
    loss, per, l1 = ops.ddm_loss_latent(c, e, d["x0"], d["noise"], d["xt"], d["t"], d["w"], schedule, use_l1)
    loss.backward()
    where = f"schedule {schedule} use_l1 {use_l1} n {n}"
    check("ddm_loss_latent", {"per": per, "l1": l1, "d_c": c.grad, "d_n": e.grad}, ref, ref32, where)
    # where an L1 argument is exactly 0 its sign is 0: the gradient there is the remaining terms alone, finite and on the bar above;
    # and with every argument 0 (C_pred = -x0 = 0 ...) it is exactly 0
    z = torch.zeros(B, 64, device="cuda")
    cz, ez = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    lz, pz, l1z = ops.ddm_loss_latent(cz, ez, z, z, z, d["t"], d["w"], schedule, use_l1)
    lz.backward()
    for v in (lz, pz, l1z, cz.grad, ez.grad):
        assert float(v.abs().max()) == 0.0, where
    runs = []
    for _ in range(2):
        p, q = (torch.full((B,), 7.0, device="cuda", dtype=torch.float64) for _ in range(2))
        hip.call("adm_ddm_loss_latent", *(hip.ptr(d[k]) for k in ("c", "e", "x0", "noise", "xt", "t", "w")), hip.ptr(p), hip.ptr(q), None,
                 None, gs, B, n, schedule, int(use_l1))
        runs.append((p.float(), q.float()))
    check("ddm_loss_latent", {"per": runs[0][0], "l1": runs[0][1]}, {k: ref[k] for k in ("per", "l1")}, ref32, "no gradients, " + where)
    if n <= 65536:
        assert all(torch.equal(a_, b_) for a_, b_ in zip(runs[0], runs[1])) and torch.equal(runs[0][0], per) and torch.equal(runs[0][1], l1)


# ------------------------------------------------------------------------------------------------ sampler steps
@pytest.mark.parametrize("scale_input", er.SCALE_INPUTS)
@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("schedule", [0, 1])
def test_sampler_step(ops, schedule, clip, last, scale_input):
    d = {k: dev(v) for k, v in er.sampler_data(er.RAGGED_N).items()}
    for tc, tn in er.SAMPLER_STEPS:
        got = ops.sampler_step(d["x"].clone(), d["c"], d["e"], tc, tn, schedule, clip, scale_input, last)
        check64("sampler_step", got, er.sampler_step(d["x"], d["c"], d["e"], tc, tn, schedule, clip, scale_input, last), er.K_SAMPLER_STEP,
                f"schedule {schedule} clip {clip} last {last} scale {scale_input} t {tc} -> {tn}")


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("schedule", [0, 1])
def test_sampler_step_stochastic(ops, schedule, clip, last):
    d = {k: dev(v) for k, v in er.sampler_data(er.RAGGED_N).items()}
    for ts in er.STOCH_TS:
        t, s = (torch.tensor([p[i] for p in ts], dtype=torch.float64, device="cuda") for i in (0, 1))
        for scale_input in er.SCALE_INPUTS:
            got = ops.sampler_step_stochastic(d["x"].clone(), d["c"], d["e"], d["z"], t, s, schedule, clip, scale_input, last)
            ref = er.sampler_step_stochastic(d["x"], d["c"], d["e"], d["z"], t, s, schedule, clip, scale_input, last)
            check64("sampler_step_stochastic", got, ref, er.K_SAMPLER_STOCHASTIC[schedule],
                    f"schedule {schedule} clip {clip} last {last} scale {scale_input} t {t.tolist()} s {s.tolist()}")
            if not last:      # s == t: sigma is exactly 0, the draw z must not enter
                b = [i for i, p in enumerate(ts) if p[0] == p[1]]
                z2 = d["z"] * 3.0 + 1.0
                got2 = ops.sampler_step_stochastic(d["x"].clone(), d["c"], d["e"], z2, t, s, schedule, clip, scale_input, last)
                assert b and torch.equal(got2[b], got[b]) and not torch.equal(got2, got)


@pytest.mark.parametrize("schedule", [0, 1])
def test_sampler_steps_wrap(ops, schedule):
    """Both steps beyond the first trip of the loop: sample 2 (its own t, s) lies wholly there."""
    d = {k: dev(v) for k, v in er.sampler_data(er.WRAP_B3).items()}
    got = ops.sampler_step(d["x"].clone(), d["c"], d["e"], 0.6, 0.45, schedule, True, 1.0, False)
    check64("sampler_step", got, er.sampler_step(d["x"], d["c"], d["e"], 0.6, 0.45, schedule, True, 1.0, False), er.K_SAMPLER_STEP, "wrap")
    t, s = (torch.tensor([p[i] for p in er.STOCH_TS[0]], dtype=torch.float64, device="cuda") for i in (0, 1))
    got = ops.sampler_step_stochastic(d["x"].clone(), d["c"], d["e"], d["z"], t, s, schedule, True, 1.0, False)
    check64("sampler_step_stochastic", got, er.sampler_step_stochastic(d["x"], d["c"], d["e"], d["z"], t, s, schedule, True, 1.0, False),
            er.K_SAMPLER_STOCHASTIC[schedule], "wrap")


# ------------------------------------------------------------------------------------------------ optimiser
def _sumsq(g, partials):
    from adm_amd import hip
    out = torch.zeros(1, device="cuda", dtype=torch.float64)
    part = torch.zeros(hip.lib().adm_sumsq_blocks(g.numel()), device="cuda", dtype=torch.float64) if partials else None
    hip.call("adm_sumsq", hip.ptr(g), hip.ptr(out), hip.ptr(part), g.numel())
    return out[0]


@pytest.mark.parametrize("partials", [True, False])
@pytest.mark.parametrize("n", [er.ADAM_N, er.ADAM_N + 1, er.ADAM_N + 2, er.ADAM_N + 3, 1, 3, er.WRAP_SUMSQ])
def test_sumsq(ops, n, partials):
    """ADAM_N + r covers the four n & 3 tails; 1 and 3 are tails alone."""
    datasets = [("uniform", dev(er.data((n,), "sumsq.g", 0.02)))]
    if n == er.ADAM_N + 1:          # one large element among tiny ones, in the body and in the tail
        for pos in (n // 2, n - 1):
            g = torch.full((n,), 1e-4, device="cuda")
            g[pos] = 1e3
            datasets.append((f"spike at {pos}", g))
    for name, g in datasets:
        got = _sumsq(g, partials)
        check("sumsq", {"sumsq": got}, er.sumsq(g), er.sumsq(g, torch.float32), f"{name} n {n} partials {partials}")
        if partials:
            assert float(_sumsq(g, True)) == float(got), "the two-stage sum must repeat bitwise"


def _adam_run(d, n, case):
    """One FusedAdamWEMA step on flat buffers of n elements (the optimiser only reads flat / grad / numel of its FlatParams)."""
    from adm_amd.optim import FusedAdamWEMA
    step, max_norm, gscale, wd, ema = case
    flat = types.SimpleNamespace(flat=d["p"].clone(), grad=d["g"].clone(), numel=n)
    opt = FusedAdamWEMA(flat, lr=er.ADAM_LR, weight_decay=wd, max_norm=max_norm, ema=ema != "none")
    opt.m, opt.v = d["m"].clone(), d["v"].clone()
    if opt.ema is not None:
        opt.ema = d["ema"].clone()
    opt.step_count = step - 1
    opt.step(grad_scale=gscale, ema_decay=None if ema == "none" else ema)
    got = {"p": flat.flat, "m": opt.m, "v": opt.v, "norm": torch.tensor(opt.grad_norm(gscale), dtype=torch.float64, device="cuda")}
    if opt.ema is not None:
        got["ema"] = opt.ema
    assert torch.equal(flat.grad, d["g"])
    return got


@pytest.mark.parametrize("case", er.ADAM_CASES + (er.ADAM_WRAP_CASE,), ids=lambda c: "-".join(str(v) for v in c))
def test_fused_adamw_ema(ops, case):
    n = er.WRAP_ADAMW if case is er.ADAM_WRAP_CASE else er.ADAM_N
    d = {k: dev(v) for k, v in er.adam_data(n).items()}
    got = _adam_run(d, n, case)
    check("adamw_step", got, er.adam_ref(d, case), er.adam_ref(d, case, torch.float32), f"n {n} case {case}")
    if case[4] == 0.0:
        exact("adamw_step", "ema (decay 0)", got["ema"], got["p"])
    if case[4] is None:
        exact("adamw_step", "ema (left alone)", got["ema"], d["ema"])


# ------------------------------------------------------------------------------------------------ layout + preconditioning
def _coef(stride, tag, B=3):
    """one coefficient (stride 0) or one per sample (stride 1), away from 1"""
    v = er.data((B,), "coef." + tag, 0.5) + 1.5
    return dev(v if stride else v[:1].clone())


LAYOUTS = [(3, 3), (3, 4), (3, 32), (6, 8)]          # (C, Cpad or ldf)


@pytest.mark.parametrize("C,cpad", LAYOUTS)
@pytest.mark.parametrize("stride", [0, 1])
@pytest.mark.parametrize("xdt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_nchw_to_nhwc(ops, xdt, stride, C, cpad):
    from adm_amd import hip
    B, H, W = 3, 5, 7
    x = dev(er.data((B, C, H, W), "l.x", 1.0, xdt))
    mul = _coef(stride, "mul")
    ref, ref32 = er.nchw_to_nhwc(x, mul, cpad), er.nchw_to_nhwc(x, mul, cpad, torch.float32)
    for amax in (False, True):
        y, s = torch.full((B, H, W, cpad), 9.0, device="cuda"), slot()
        if amax:
            hip.call("adm_nchw_to_nhwc_amax", hip.ptr(x), int(xdt == torch.float64), hip.ptr(mul), stride, hip.ptr(y), hip.ptr(s), B, C, H * W, cpad)
            check_bound("nchw_to_nhwc_amax", s, y)
        else:
            hip.call("adm_nchw_to_nhwc", hip.ptr(x), int(xdt == torch.float64), hip.ptr(mul), stride, hip.ptr(y), B, C, H * W, cpad)
        check("nchw_to_nhwc", {"y": y}, ref, ref32, f"{xdt} stride {stride} C {C} cpad {cpad} amax {amax}")
        assert float(y[..., C:].abs().sum()) == 0.0, "pad channels must be exactly 0"
    # coefficient 1 (mul NULL): a transpose; then the wrapper with its gradient to x (the scaled NHWC -> NCHW transpose)
    y = torch.full((B, H, W, cpad), 9.0, device="cuda")
    hip.call("adm_nchw_to_nhwc", hip.ptr(x), int(xdt == torch.float64), None, 0, hip.ptr(y), B, C, H * W, cpad)
    exact("nchw_to_nhwc", "y (coefficient 1)", y, er.nchw_to_nhwc(x.float(), None, cpad)["y"][0])
    xg = x.clone().requires_grad_(True)
    yw = ops.nchw_to_nhwc(xg, mul, cpad)
    check("nchw_to_nhwc", {"y": yw}, ref, ref32, "wrapper")
    dy = dev(er.data((B, H, W, cpad), "l.dy", 1.0))
    yw.backward(dy)
    assert xg.grad.dtype == xdt
    check("precond_out", {"out": xg.grad}, er.precond_out(None, dy, None, mul, C), er.precond_out(None, dy, None, mul, C, torch.float32),
          "x NULL: gradient of nchw_to_nhwc")


@pytest.mark.parametrize("C,ldf", LAYOUTS)
@pytest.mark.parametrize("stride", [0, 1])
@pytest.mark.parametrize("xdt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_precond_out_and_gradients(ops, xdt, stride, C, ldf):
    from adm_amd import hip
    B, H, W = 3, 5, 7
    x = dev(er.data((B, C, H, W), "p.x", 1.0, xdt))
    f = dev(er.data((B, H, W, ldf), "p.f", 1.3))
    a, s = _coef(stride, "a"), _coef(stride, "s")
    fg, xg = f.clone().requires_grad_(True), x.clone().requires_grad_(True)
    out = ops.precond_out(fg, xg, a, s)
    check("precond_out", {"out": out}, er.precond_out(x, f, a, s, C), er.precond_out(x, f, a, s, C, torch.float32),
          f"{xdt} stride {stride} C {C} ldf {ldf}")
    dout = dev(er.data((B, C, H, W), "p.dout", 1.0))
    out.backward(dout)           # df through precond_out_bwd[_amax] (pad channels 0), dx through axpby_b with x NULL
    check("precond_out_bwd", {"df": fg.grad}, er.precond_out_bwd(dout, s, ldf), er.precond_out_bwd(dout, s, ldf, torch.float32), "df")
    assert float(fg.grad[..., C:].abs().sum()) == 0.0 and xg.grad.dtype == xdt
    check("axpby_b", {"out": xg.grad}, er.axpby_b(None, dout, None, a), er.axpby_b(None, dout, None, a, torch.float32), "x NULL: dx of precond_out")
    # x NULL and s = 1: the plain transpose
    one, o = torch.ones(1, device="cuda"), torch.full((B, C, H, W), 9.0, device="cuda")
    hip.call("adm_precond_out", None, 0, hip.ptr(f), ldf, None, hip.ptr(one), 0, hip.ptr(o), B, C, H * W)
    exact("precond_out", "out (x NULL, coefficient 1)", o, er.precond_out(None, f, None, one, C)["out"][0])
    # both entry points of the gradient, with and without the bound vector
    for amax in (False, True):
        df, sl = torch.full((B, H, W, ldf), 9.0, device="cuda"), slot()
        if amax:
            hip.call("adm_precond_out_bwd_amax", hip.ptr(dout), hip.ptr(s), stride, hip.ptr(df), ldf, hip.ptr(sl), B, C, H * W)
            check_bound("precond_out_bwd_amax", sl, df)
        else:
            hip.call("adm_precond_out_bwd", hip.ptr(dout), hip.ptr(s), stride, hip.ptr(df), ldf, B, C, H * W)
        check("precond_out_bwd", {"df": df}, er.precond_out_bwd(dout, s, ldf), er.precond_out_bwd(dout, s, ldf, torch.float32), f"amax {amax}")
        assert float(df[..., C:].abs().sum()) == 0.0


@pytest.mark.parametrize("stride", [0, 1])
@pytest.mark.parametrize("xdt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_axpby_b_and_gradients(ops, xdt, stride):
    B, n = 3, er.RAGGED_N
    x, y = dev(er.data((B, n), "ax.x", 1.0, xdt)), dev(er.data((B, n), "ax.y", 1.3))
    a, s = _coef(stride, "a"), _coef(stride, "s")
    yg, xg = y.clone().requires_grad_(True), x.clone().requires_grad_(True)
    out = ops.axpby_batch(yg, xg, a, s)
    check("axpby_b", {"out": out}, er.axpby_b(x, y, a, s), er.axpby_b(x, y, a, s, torch.float32), f"{xdt} stride {stride}")
    dout = dev(er.data((B, n), "ax.dout", 1.0))
    out.backward(dout)
    check("axpby_b", {"out": yg.grad}, er.axpby_b(None, dout, None, s), er.axpby_b(None, dout, None, s, torch.float32), "dy")
    check("axpby_b", {"out": xg.grad}, er.axpby_b(None, dout, None, a), er.axpby_b(None, dout, None, a, torch.float32), "dx")
    assert xg.grad.dtype == xdt


@pytest.mark.parametrize("C", [3, 6])
@pytest.mark.parametrize("ldf", [8, 32])
def test_head_out_and_gradient(ops, ldf, C):
    """nhwc_to_nchw (csrc/ddm_linear.hip) and its adjoint with the bound vector: pure data movement."""
    from adm_amd import hip
    B, H, W = 3, 5, 7
    f = dev(er.data((B, H, W, ldf), "h.f", 1.3)).requires_grad_(True)
    out = ops.head_out(f, C)
    exact("nhwc_to_nchw", "out", out.detach(), f.detach()[..., :C].permute(0, 3, 1, 2).contiguous())
    dout = dev(er.data((B, C, H, W), "h.dout", 1.0))
    out.backward(dout)
    want = er.precond_out_bwd(dout, None, ldf)["df"][0]
    exact("nhwc_to_nchw_bwd_amax", "df", f.grad, want)
    df, sl = torch.full((B, H, W, ldf), 9.0, device="cuda"), slot()
    hip.call("adm_nhwc_to_nchw_bwd_amax", hip.ptr(dout), hip.ptr(df), ldf, hip.ptr(sl), B, C, H * W)
    exact("nhwc_to_nchw_bwd_amax", "df", df, want)
    check_bound("nhwc_to_nchw_bwd_amax", sl, df)


def test_layout_kernels_wrap(ops):
    """B HW (nchw_to_nhwc, precond_out_bwd: one thread per pixel) and B C HW (precond_out, axpby_b) just above the grid cap, Cpad = 4,
    per-sample coefficients: sample 2 lies beyond the first trip."""
    from adm_amd import hip
    B, C, cpad = 3, 3, 4
    HW = er.WRAP_B3
    x, mul = dev(er.data((B, C, 1, HW), "lw.x", 1.0)), _coef(1, "mul")
    y, sl = torch.full((B, 1, HW, cpad), 9.0, device="cuda"), slot()
    hip.call("adm_nchw_to_nhwc_amax", hip.ptr(x), 0, hip.ptr(mul), 1, hip.ptr(y), hip.ptr(sl), B, C, HW, cpad)
    check("nchw_to_nhwc", {"y": y}, er.nchw_to_nhwc(x, mul, cpad), er.nchw_to_nhwc(x, mul, cpad, torch.float32), "wrap")
    check_bound("nchw_to_nhwc_amax", sl, y)
    assert float(y[..., C:].abs().sum()) == 0.0
    df, sl = torch.full((B, 1, HW, cpad), 9.0, device="cuda"), slot()
    hip.call("adm_precond_out_bwd_amax", hip.ptr(x), hip.ptr(mul), 1, hip.ptr(df), cpad, hip.ptr(sl), B, C, HW)
    check("precond_out_bwd", {"df": df}, er.precond_out_bwd(x, mul, cpad), er.precond_out_bwd(x, mul, cpad, torch.float32), "wrap")
    check_bound("precond_out_bwd_amax", sl, df)
    hw = (er.WRAP_1 + 8) // 9
    xs, f = dev(er.data((B, C, 1, hw), "lw.xs", 1.0, torch.float64)), dev(er.data((B, 1, hw, cpad), "lw.f", 1.3))
    a, s = _coef(1, "a"), _coef(1, "s")
    out = ops.precond_out(f, xs, a, s)
    check("precond_out", {"out": out}, er.precond_out(xs, f, a, s, C), er.precond_out(xs, f, a, s, C, torch.float32), "wrap")
    xa, ya = dev(er.data((B, er.WRAP_B3), "lw.xa", 1.0)), dev(er.data((B, er.WRAP_B3), "lw.ya", 1.3))
    out = ops.axpby_batch(ya, xa, a, s)
    check("axpby_b", {"out": out}, er.axpby_b(xa, ya, a, s), er.axpby_b(xa, ya, a, s, torch.float32), "wrap")


# ------------------------------------------------------------------------------------------------ resample, concat, copy, add, silu, embedding
def _resample(x, mode, scale, prefill):
    from adm_amd import hip
    B, H, W, C = x.shape
    y = torch.full((B, H // 2, W // 2, C) if mode == 0 else (B, 2 * H, 2 * W, C), 9.0, device="cuda") if prefill is None else prefill.clone()
    hip.call("adm_resample2x", hip.ptr(x), hip.ptr(y), B, H, W, C, mode, scale, int(prefill is not None))
    return y


@pytest.mark.parametrize("C", [4, 36])
@pytest.mark.parametrize("mode", [0, 1])
def test_resample2x(ops, mode, C):
    from adm_amd import hip
    B, H, W = 3, 6, 10
    x = dev(er.data((B, H, W, C), "r.x", 1.0))
    oshape = (B, H // 2, W // 2, C) if mode == 0 else (B, 2 * H, 2 * W, C)
    pre = dev(er.data(oshape, "r.pre", 1.0))
    for scale in (0.25, 1.0):
        for prefill in (None, pre):
            got = _resample(x, mode, scale, prefill)
            where = f"mode {mode} C {C} scale {scale} acc {int(prefill is not None)}"
            if mode == 1 and scale == 1.0 and prefill is None:
                exact("resample2x", "y (up2x, scale 1)", got, er.resample2x(x.float(), 1, 1.0)["y"][0])
            check("resample2x", {"y": got}, er.resample2x(x, mode, scale, prefill), er.resample2x(x, mode, scale, prefill, torch.float32), where)
    # the wrappers with their gradients (down: up x 0.25; up: the 2x2 sum)
    xg = x.clone().requires_grad_(True)
    y = ops.downsample2x(xg) if mode == 0 else ops.upsample2x(xg)
    check("resample2x", {"y": y}, er.resample2x(x, mode, 0.25 if mode == 0 else 1.0), er.resample2x(x, mode, 0.25 if mode == 0 else 1.0, None, torch.float32), "wrapper")
    y.backward(pre)
    a = (pre, 1 - mode, 0.25 if mode == 0 else 1.0)
    check("resample2x", {"y": xg.grad}, er.resample2x(*a), er.resample2x(*a, None, torch.float32), "wrapper gradient")
    # rejected shapes
    lib = hip.lib()
    bad = lambda *a_: lib.adm_resample2x(hip.ptr(x), hip.ptr(pre), *a_, hip.stream())
    assert bad(B, 5, W, C, 0, 1.0, 0) == -22 and bad(B, H, 9, C, 0, 1.0, 0) == -22 and bad(B, H, W, C - 2, 1, 1.0, 0) == -22
    assert bad(B, H, W, C - 1, 0, 1.0, 0) == -22 and bad(B, H, W, C, 2, 1.0, 0) == -22


def test_resample2x_wrap(ops):
    """Output vectors (16 bytes each) just above the grid cap, both modes, C = 4."""
    wo = er.WRAP_X4 // 3 + 1
    x = dev(er.data((3, 2, 2 * wo, 4), "rw.x", 1.0))
    check("resample2x", {"y": _resample(x, 0, 0.25, None)}, er.resample2x(x, 0, 0.25), er.resample2x(x, 0, 0.25, None, torch.float32), "wrap down")
    del x
    wi = er.WRAP_X4 // 12 + 1
    x = dev(er.data((3, 1, wi, 4), "rw.xu", 1.0))
    got = _resample(x, 1, 1.0, None)
    exact("resample2x", "y (up2x, scale 1)", got, er.resample2x(x.float(), 1, 1.0)["y"][0])
    pre = dev(er.data(tuple(got.shape), "rw.pre", 1.0))
    check("resample2x", {"y": _resample(x, 1, 0.25, pre)}, er.resample2x(x, 1, 0.25, pre), er.resample2x(x, 1, 0.25, pre, torch.float32), "wrap up acc")


@pytest.mark.parametrize("M,ca,cb", [(3 * 35, 8, 4), (107, 36, 4), (er.WRAP_X4 // 3 + 1, 4, 8)])
def test_concat2_split2(ops, M, ca, cb):
    from adm_amd import hip
    a, b = dev(er.data((M, ca), "c.a", 1.0)), dev(er.data((M, cb), "c.b", 1.3))
    for scale_b in (1.0, 0.7071067811865476):
        sb = er.f32(scale_b)
        y, sl = torch.full((M, ca + cb), 9.0, device="cuda"), slot()
        hip.call("adm_concat2", hip.ptr(a), ca, hip.ptr(b), cb, hip.ptr(y), M, sb, hip.ptr(sl))
        check_bound("concat2", sl, y)
        dy = dev(er.data((M, ca + cb), "c.dy", 1.0))
        da, db = torch.full((M, ca), 9.0, device="cuda"), torch.full((M, cb), 9.0, device="cuda")
        hip.call("adm_split2", hip.ptr(dy), hip.ptr(da), ca, hip.ptr(db), cb, M, sb)
        if scale_b == 1.0:
            exact("concat2", "y (scale 1)", y, torch.cat([a, b], dim=1))
            exact("split2", "da", da, dy[:, :ca])
            exact("split2", "db (scale 1)", db, dy[:, ca:])
        else:
            check("concat2", {"y": y}, er.concat2(a, b, sb), er.concat2(a, b, sb, torch.float32), f"M {M} {ca}+{cb}")
            check("split2", {"da": da, "db": db}, er.split2(dy, ca, sb), er.split2(dy, ca, sb, torch.float32), f"M {M} {ca}+{cb}")
    if M < 1000:          # the wrapper (bound vector or none, as the switches say) and its gradient
        ag, bg = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = ops.concat_channels(ag, bg, 1.0)
        exact("concat2", "y (scale 1)", y.detach(), torch.cat([a, b], dim=1))
        y.backward(dy)
        exact("split2", "da", ag.grad, dy[:, :ca])
        exact("split2", "db (scale 1)", bg.grad, dy[:, ca:])


@pytest.mark.parametrize("M", [107, er.WRAP_X4 // 2 + 1])
def test_copy_channels(ops, M):
    """No caller in the package: the entry point as the header documents it.  Offsets and leading dimensions above C, with acc."""
    from adm_amd import hip
    C, lds, so, ldd, do = 8, 20, 8, 16, 4
    src, dst0 = dev(er.data((M, lds), "cc.src", 1.0)), dev(er.data((M, ldd), "cc.dst", 1.3))
    for scale, acc in ((1.0, 0), (0.37, 0), (1.0, 1), (0.37, 1)):
        dst, sc = dst0.clone(), er.f32(scale)
        hip.call("adm_copy_channels", hip.ptr(src), lds, so, hip.ptr(dst), ldd, do, M, C, sc, acc)
        a = (src, so, dst0, do, C, sc, acc)
        if scale == 1.0 and not acc:
            exact("copy_channels", "dst (scale 1)", dst, er.copy_channels(src, so, dst0, do, C, 1.0, 0, torch.float32)["dst"][0])
        check("copy_channels", {"dst": dst}, er.copy_channels(*a), er.copy_channels(*a, torch.float32), f"M {M} scale {scale} acc {acc}")
        keep = torch.ones(ldd, dtype=torch.bool, device="cuda")
        keep[do:do + C] = False
        assert torch.equal(dst[:, keep], dst0[:, keep]), "columns outside the copied channels must stay"
    lib = hip.lib()
    assert lib.adm_copy_channels(hip.ptr(src), lds, so, hip.ptr(dst), ldd, do, M, 6, 1.0, 0, hip.stream()) == -22
    assert lib.adm_copy_channels(hip.ptr(src), lds, 2, hip.ptr(dst), ldd, do, M, C, 1.0, 0, hip.stream()) == -22


@pytest.mark.parametrize("n", [3 * er.RAGGED_N, er.WRAP_1])
def test_add_silu(ops, n):
    from adm_amd import hip
    a, b = dev(er.data((n,), "a.a", 1.0)), dev(er.data((n,), "a.b", 1.3))
    y = torch.full((n,), 9.0, device="cuda")
    hip.call("adm_add", hip.ptr(a), hip.ptr(b), hip.ptr(y), n)
    check("add", {"y": y}, er.add(a, b), er.add(a, b, None, torch.float32), f"n {n}")
    x = dev(er.data((n,), "a.x", 12.0))
    x[:8] = torch.tensor([-100.0, 100.0, -88.0, 88.0, -20.0, 20.0, 0.0, -0.0], device="cuda")
    x[-2:] = torch.tensor([-100.0, 100.0], device="cuda")
    xg = x.clone().requires_grad_(True)
    ys = ops.silu(xg)
    ys.backward(b)
    check("silu", {"y": ys, "dx": xg.grad}, er.silu(x, b), er.silu(x, b, torch.float32), f"n {n}")
    g = xg.grad / b          # the gradient goes to 0 (x -> -inf) or 1 (x -> +inf)
    assert float(g[0].abs()) <= 1e-30 and float(g[-2].abs()) <= 1e-30 and float(g[1]) == 1.0 and float(g[-1]) == 1.0
    assert float(ys[0].abs()) <= 1e-30 and float(ys[1]) == 100.0


@pytest.mark.parametrize("n4", [3 * er.RAGGED_N, er.WRAP_X4])
def test_add3(ops, n4):
    from adm_amd import hip
    n = 4 * n4
    a, b, c = (dev(er.data((n,), "a3." + k, s)) for k, s in (("a", 1.0), ("b", 1.3), ("c", 0.7)))
    for third in (c, None):
        y, sl = torch.full((n,), 9.0, device="cuda"), slot()
        hip.call("adm_add3", hip.ptr(a), hip.ptr(b), hip.ptr(third), hip.ptr(y), hip.ptr(sl), n)
        check("add3", {"y": y}, er.add(a, b, third), er.add(a, b, third, torch.float32), f"n {n} c {third is not None}")
        check_bound("add3", sl, y)
    y2 = torch.full((n,), 9.0, device="cuda")
    hip.call("adm_add3", hip.ptr(a), hip.ptr(b), hip.ptr(c), hip.ptr(y2), None, n)          # no bound vector
    assert torch.equal(y2, (a + b) + c)
    assert hip.lib().adm_add3(hip.ptr(a), hip.ptr(b), None, hip.ptr(y2), None, n - 1, hip.stream()) == -22


def test_fanout_gradient_sum(ops):
    """ops.fanout: three consumers -> one add3; a size that is no multiple of 4 -> add."""
    for shape in ((3, 5, 7, 4), (3, 5, 7, 3)):
        x = dev(er.data(shape, "f.x", 1.0)).requires_grad_(True)
        gs = [dev(er.data(shape, f"f.g{i}", 1.0 + i)) for i in range(3)]
        outs = ops.fanout(x, 3)
        (sum((o * g).sum() for o, g in zip(outs, gs))).backward()
        check("add3" if shape[-1] == 4 else "add", {"y": x.grad}, er.add(*gs), er.add(*gs, torch.float32), f"fanout {shape}")


@pytest.mark.parametrize("C", [2, 192])
def test_pos_embedding(ops, C):
    import math
    for t in ([math.log(1e-4), math.log(1e-4) / 4, 0.0], [-1.0, math.log(0.999) / 4, -5.5]):
        t = torch.tensor(t, dtype=torch.float32, device="cuda")
        got = ops.pos_embedding(t, C)
        check("pos_embedding", {"emb": got}, er.pos_embedding(t, C), er.pos_embedding(t, C, torch.float32), f"C {C} t {t.tolist()}")


# ------------------------------------------------------------------------------------------------ bound vectors
def _producers():
    """name -> (run(x [3, n4 * 4 floats as the producer shapes them], slot) -> y, how many floats of x per 'n4')"""
    from adm_amd import hip
    one = torch.ones(1, device="cuda")

    def nchw(x, sl):          # x [3, 4, HW] -> y [3, HW, 4]
        B, C, HW = x.shape
        y = torch.empty(B, HW, C, device="cuda")
        hip.call("adm_nchw_to_nhwc_amax", hip.ptr(x), 0, hip.ptr(one), 0, hip.ptr(y), hip.ptr(sl), B, C, HW, C)
        return y

    def pbwd(x, sl):
        B, C, HW = x.shape
        y = torch.empty(B, HW, C, device="cuda")
        hip.call("adm_precond_out_bwd_amax", hip.ptr(x), hip.ptr(one), 0, hip.ptr(y), C, hip.ptr(sl), B, C, HW)
        return y

    def hbwd(x, sl):
        B, C, HW = x.shape
        y = torch.empty(B, HW, C, device="cuda")
        hip.call("adm_nhwc_to_nchw_bwd_amax", hip.ptr(x), hip.ptr(y), C, hip.ptr(sl), B, C, HW)
        return y

    def add3(x, sl):
        y, z = torch.empty_like(x), torch.zeros_like(x)
        hip.call("adm_add3", hip.ptr(x), hip.ptr(z), hip.ptr(z), hip.ptr(y), hip.ptr(sl), x.numel())
        return y

    def cat(x, sl):           # a = zeros [M, 4], b = x as [M, 8]: the last element of x is the last of y
        b = x.reshape(-1, 8)
        a = torch.zeros(b.shape[0], 4, device="cuda")
        y = torch.empty(b.shape[0], 12, device="cuda")
        hip.call("adm_concat2", hip.ptr(a), 4, hip.ptr(b), 8, hip.ptr(y), b.shape[0], 1.0, hip.ptr(sl))
        return y

    return {"nchw_to_nhwc_amax": nchw, "precond_out_bwd_amax": pbwd, "nhwc_to_nchw_bwd_amax": hbwd, "add3": add3, "concat2": cat}


@pytest.mark.parametrize("name", ["nchw_to_nhwc_amax", "precond_out_bwd_amax", "nhwc_to_nchw_bwd_amax", "add3", "concat2"])
def test_bound_vector_producers(ops, name):
    """max |y| in element 0, in the very last element of a ragged total, and beyond the first trip of the grid-stride loop (the one
    kernel without such a loop, nhwc_to_nchw_bwd, gets the same sizes); an all-zero output leaves the vector as it was."""
    run = _producers()[name]
    small = torch.zeros(3, 4, 2 * 35 + 1 if name != "concat2" else 70, device="cuda")          # 3 x 71 pixels; concat2 needs rows of 8
    big_hw = er.WRAP_B3 if name in ("nchw_to_nhwc_amax", "precond_out_bwd_amax") else (er.WRAP_X4 * 4 // 12 // 8 + 1) * 8
    for x, pos in ((small, 0), (small, small.numel() - 1), (torch.zeros(3, 4, big_hw, device="cuda"), -1)):
        x = x.clone()
        x.view(-1)[:] = dev(er.data((x.numel(),), "bound." + name, 0.5))
        if pos == -1:          # the last pixel of the last sample's first channel row ... any element past the first trip: take the last
            pos = x.numel() - 1
        x.view(-1)[pos] = -7.25
        sl = slot()
        y = run(x, sl)
        assert float(y.abs().max()) == 7.25 and float(sl.max()) == 7.25 and float(sl.min()) >= 0.0, (name, pos, float(sl.max()))
    sl = slot(0.5)
    sl[::3] = 0.0
    before = sl.clone()
    y = run(torch.zeros_like(small), sl)
    assert float(y.abs().max()) == 0.0 and torch.equal(sl, before), name


# ------------------------------------------------------------------------------------------------ the record
def test_zz_report_worst_errors():
    """Worst e_max / e_rms per kernel and output, with the largest ratio to its limit (the table of profiles/elementwise_errors.md:
    written to the path in ADM_ELEMENTWISE_REPORT when that is set)."""
    if not WORST:
        pytest.skip("no case ran in this session")
    lines = ["| kernel | output | bar | worst e_max | worst e_rms | worst ratio to the limit |", "|---|---|---|---|---|---|"]
    for (kernel, out), (em, er_, ratio, bar) in sorted(WORST.items()):
        lines.append(f"| {kernel} | {out} | {bar} | {em:.3e} | {er_:.3e} | {ratio:.3f} |")
    print("\nworst error vs fp64 per kernel / output:\n" + "\n".join(lines))
    path = os.environ.get("ADM_ELEMENTWISE_REPORT")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
