"""CPU: the float64 references of tests/elementwise_ref.py against independent statements of the same operations (autograd of the
loss, the oracle's schedule and samplers, torch.optim.AdamW + clip_grad_norm_ + lerp_, torch's pooling / interpolation / cat), and
the conditions tests/test_hip_elementwise.py relies on: the data it uses does what its docstrings say, and plain fp32 torch stays
under BAR_A / 4 on all of it, so the ceiling BAR_A never decides a case there (no GPU needed)."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import ddm_ref

import elementwise_ref as er
import fp64ref
from test_hip_accuracy import BAR_A

_f64 = torch.float64
SCHED = ("const", "const_2")


def near(a, b, tol=1e-13):
    a, b = a.double(), b.double()
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def e32_ok(ref, ref32, where):
    """plain fp32 torch is under BAR_A / 4 on this data"""
    for n, (r, mag) in ref.items():
        e = fp64ref.errors(ref32[n][0], r, mag)
        assert e[0] <= BAR_A / 4, (where, n, e)


# ------------------------------------------------------------------------------------------------ schedule and loss
@pytest.mark.parametrize("schedule", [0, 1])
def test_q_sample_and_weights_match_the_oracle(schedule):
    x0, noise = er.data((3, er.RAGGED_N), "q.x0", 1.0, _f64), er.data((3, er.RAGGED_N), "q.noise", 1.7, _f64)
    seen = set()
    for t in er.t_triples():
        seen |= {round(float(v), 6) for v in t}
        ref = er.q_sample(x0, noise, t, schedule)
        near(ref["xt"][0], ddm_ref.q_sample(SCHED[schedule], x0, noise, t.double(), -x0))
        assert bool((ref["xt"][1] >= ref["xt"][0].abs() - 1e-15).all())
        e32_ok(ref, er.q_sample(x0, noise, t, schedule, torch.float32), f"q_sample {schedule} {t}")
    assert {round(v, 6) for v in er.T_CASES} <= seen
    t = er.loss_data(er.RAGGED_N, schedule)["t"]
    assert len(set(t.tolist())) == er.LOSS_B and float(t.min()) < 1e-4 and float(t.max()) == float(torch.tensor(0.999))
    w = er.loss_weights(schedule, t)
    w1, w2 = ddm_ref.loss_weights(SCHED[schedule], t.double(), er.LOSS_EPS)
    near(w[:, 0], w1.float()), near(w[:, 1], w2.float()), near(w[:, 2], (-torch.log(t.double()) / 2).float())
    assert min(er.LOSS_T) == 1e-4 and max(er.LOSS_T) == 0.999


@pytest.mark.parametrize("n", er.LOSS_NS)
@pytest.mark.parametrize("schedule", [0, 1])
def test_loss_references_match_autograd_and_data_is_as_promised(schedule, n):
    d = er.loss_data(n, schedule)
    B = er.LOSS_B
    gs = er.f32(1.0 / B)
    c, e = d["c"].double().requires_grad_(True), d["e"].double().requires_grad_(True)
    x0, noise, xt, w = d["x0"].double(), d["noise"].double(), d["xt"].double(), d["w"].double()
    t = d["t"].double().reshape(B, 1)
    g = torch.sqrt(t) if schedule == 0 else t
    # the data: exact zeros of every L1 argument, and everything else away from zero by more than fp32 rounding can move it
    e1, e2, dd = (c + x0).detach(), (e - noise).detach(), (xt - c * t - g * e - x0).detach()
    for v, lo in ((e1, 0.0), (e2, 0.0), (dd, 5e-3)):
        assert int((v == 0).sum()) >= n // 20 and float(v[v != 0].abs().min()) > lo
    d32 = ((d["xt"] - d["c"] * d["t"].reshape(B, 1)) - (torch.sqrt(d["t"]) if schedule == 0 else d["t"]).reshape(B, 1) * d["e"]) - d["x0"]
    assert torch.equal(torch.sign(d32).double(), torch.sign(dd))
    # ddm_loss
    ref = er.ddm_loss(d["c"], d["e"], d["x0"], d["noise"], d["w"][:, :2], gs)
    per = w[:, 0] * ((c + x0) ** 2).sum(1) + w[:, 1] * ((e - noise) ** 2).sum(1)
    gc, gn = torch.autograd.grad(per.sum() * gs, (c, e))
    near(ref["per"][0], per.detach()), near(ref["d_c"][0], gc), near(ref["d_n"][0], gn)
    e32_ok(ref, er.ddm_loss(d["c"], d["e"], d["x0"], d["noise"], d["w"][:, :2], gs, torch.float32), f"ddm_loss {schedule} {n}")
    # ddm_loss_latent, as ddm_const_2.py's p_losses states it
    for use_l1 in (False, True):
        a = (d["c"], d["e"], d["x0"], d["noise"], d["xt"], d["t"], d["w"], gs, schedule, use_l1)
        ref = er.ddm_loss_latent(*a)
        simple = w[:, 0] * ((c + x0) ** 2).sum(1) + w[:, 1] * ((e - noise) ** 2).sum(1)
        if use_l1:
            simple = (simple + w[:, 0] * (c + x0).abs().sum(1) + w[:, 1] * (e - noise).abs().sum(1)) / 2
        x_rec = xt - c * t - g * e
        l1 = (x_rec - x0).abs().sum(1)
        gc, gn = torch.autograd.grad((simple.sum() + (l1 * w[:, 2]).sum()) * gs, (c, e))
        near(ref["per"][0], simple.detach()), near(ref["l1"][0], l1.detach()), near(ref["d_c"][0], gc), near(ref["d_n"][0], gn)
        for k in ref:
            assert bool((ref[k][1] >= ref[k][0].abs() * (1 - 1e-12)).all()), k
        e32_ok(ref, er.ddm_loss_latent(*a, torch.float32), f"ddm_loss_latent {schedule} {use_l1} {n}")


# ------------------------------------------------------------------------------------------------ sampler steps
@pytest.mark.parametrize("scale_input", er.SCALE_INPUTS)
@pytest.mark.parametrize("schedule", [0, 1])
def test_sampler_references_match_the_oracle(schedule, scale_input):
    """Whole runs of the oracle's samplers with a model that returns fixed (C, eps), against the references chained step by step; and
    the oracle's own statement of one stochastic step on float64 t, s.  (sample_fn_s keeps t and s of 'const_2' in float32, as the
    reference does, and so forms (2 s t - s^2) / t and C t in float32: that run agrees to float32 rounding only.)"""
    d = er.sampler_data(er.RAGGED_N)
    model = lambda x, t, **k: (d["c"], d["e"])
    for ts in er.STOCH_TS:
        t, s = (torch.tensor([p[i] for p in ts], dtype=_f64) for i in (0, 1))
        for clip in (False, True):
            x0 = ddm_ref.pred_x0_from_xt(SCHED[schedule], d["x"], d["e"].double(), d["c"].double(), t)
            x0 = x0.clamp(-scale_input, scale_input) if clip else x0
            want = ddm_ref.pred_xtms_from_xt(SCHED[schedule], d["x"], d["e"].double(), -x0, t, s, d["z"])
            near(er.sampler_step_stochastic(d["x"], d["c"], d["e"], d["z"], t, s, schedule, clip, scale_input, False)["x"][0], want)
            want = (want.clamp(-scale_input, scale_input) / scale_input + 1) * 0.5
            near(er.sampler_step_stochastic(d["x"], d["c"], d["e"], d["z"], t, s, schedule, clip, scale_input, True)["x"][0], want)
    n = 4
    for clip in (False, True):
        # deterministic: sample_fn_d clamps x0 in 'const' only
        ts = ddm_ref.t_steps_deterministic(SCHED[schedule], n, 0.01, 1.0)
        want = ddm_ref.sample_fn_d(SCHED[schedule], model, d["x"], n, 0.01, 1.0, scale_input, clip)
        x = d["x"] * ts[0]
        for i in range(n):
            x = er.sampler_step(x, d["c"], d["e"], float(ts[i]), float(ts[i + 1]), schedule, clip and schedule == 0, scale_input, i == n - 1)["x"][0]
        near(x, want, 1e-12)
        # stochastic: per-step draws injected; the last step has s == t
        eps = [er.data((3, er.RAGGED_N), f"smp.eps{i}", 2.0, _f64) for i in range(n)]
        want = ddm_ref.sample_fn_s(SCHED[schedule], model, d["x"], eps, n, 0.01, 1.0, scale_input, clip)
        grid = torch.cat([1.0 + torch.arange(n, dtype=_f64) / (n - 1) * (0.01 ** 2 - 1.0), torch.zeros(1, dtype=_f64)])
        steps = -torch.diff(grid)
        x = d["x"].float().double() if schedule == 0 else d["x"].clone()          # ('const' starts from the float32 draw)
        cur = torch.ones(3, dtype=_f64 if schedule == 0 else torch.float32)
        for i in range(n):
            s = torch.full((3,), float(steps[i]), dtype=torch.float32) if i < n - 1 else cur
            x = er.sampler_step_stochastic(x, d["c"], d["e"], eps[i], cur.double(), s.double(), schedule, clip, scale_input, i == n - 1)["x"][0]
            cur = cur - s
        near(x, want, 1e-12 if schedule == 0 else 5e-6)


@pytest.mark.parametrize("schedule", [0, 1])
def test_sampler_cases_are_finite(schedule):
    """Every (t, s) pair the GPU file uses: finite reference, sigma exactly 0 where s == t (the draw does not enter), mag >= |x|."""
    d = er.sampler_data(er.RAGGED_N)
    assert any(tn == 0.0 for _, tn in er.SAMPLER_STEPS) and (1e-4, 0.0) in er.SAMPLER_STEPS
    for tc, tn in er.SAMPLER_STEPS:
        for last in (False, True):
            r, m = er.sampler_step(d["x"], d["c"], d["e"], tc, tn, schedule, True, er.SCALE_INPUTS[1], last)["x"]
            assert bool(torch.isfinite(r).all()) and bool((m >= r.abs() * (1 - 1e-12)).all())
    same = 0
    for ts in er.STOCH_TS:
        t, s = (torch.tensor([p[i] for p in ts], dtype=_f64) for i in (0, 1))
        assert len(set(t.tolist())) == 3 and bool((s <= t).all())
        for last in (False, True):
            a = (d["x"], d["c"], d["e"])
            r, m = er.sampler_step_stochastic(*a, d["z"], t, s, schedule, True, er.SCALE_INPUTS[1], last)["x"]
            assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(m).all()) and bool((m >= r.abs() * (1 - 1e-12)).all())
            r2 = er.sampler_step_stochastic(*a, d["z"] * 3 + 1, t, s, schedule, True, er.SCALE_INPUTS[1], last)["x"][0]
            eq = [i for i, p in enumerate(ts) if p[0] == p[1]]
            assert eq and torch.equal(r2[eq], r[eq])
            same += len(eq)
    assert same and any(p[0] == 1e-4 for ts in er.STOCH_TS for p in ts)


# ------------------------------------------------------------------------------------------------ optimiser
@pytest.mark.parametrize("max_norm", [0.0, 0.05, 10.0])
@pytest.mark.parametrize("wd,gscale,ema_decay", [(0.0, 1.0, 0.9996), (1e-2, 0.125, 0.9)])
def test_optimiser_reference_matches_torch_adamw(max_norm, wd, gscale, ema_decay):
    """Five steps of torch.optim.AdamW + clip_grad_norm_ + lerp_ in float64 against the reference chained on its own outputs."""
    d = {k: v.double() for k, v in er.adam_data(er.ADAM_N).items()}
    p = torch.nn.Parameter(d["p"].clone())
    opt = torch.optim.AdamW([p], lr=er.ADAM_LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    ema = d["ema"].clone()
    mine = dict(p=d["p"], m=torch.zeros_like(d["p"]), v=torch.zeros_like(d["p"]), ema=d["ema"])
    for step in range(1, 6):
        g = er.data((er.ADAM_N,), f"adam.g{step}", 0.02, _f64)
        p.grad = g * gscale
        norm = torch.nn.utils.clip_grad_norm_([p], max_norm) if max_norm > 0 else torch.linalg.vector_norm(p.grad)
        opt.step()
        ema.lerp_(p.detach(), 1 - ema_decay)
        r = er.adamw_ema_step(mine["p"], g, mine["m"], mine["v"], mine["ema"], step=step, lr=er.ADAM_LR, weight_decay=wd, max_norm=max_norm,
                              grad_scale=gscale, ema_decay=ema_decay)
        mine = {k: r[k][0] for k in ("p", "m", "v", "ema")}
        near(r["norm"][0], norm.detach(), 1e-12)
        st = opt.state[p]
        near(mine["p"], p.detach(), 1e-12), near(mine["m"], st["exp_avg"], 1e-12), near(mine["v"], st["exp_avg_sq"], 1e-12), near(mine["ema"], ema, 1e-12)
        for k in ("p", "m", "v", "ema"):
            assert bool((r[k][1] >= r[k][0].abs() * (1 - 1e-12)).all())
    if max_norm:       # the clip did what the case is there for
        assert (float(norm) > max_norm) == (max_norm == 0.05)


def test_optimiser_cases():
    """The cases of the GPU file: every step count, clip off / inactive / active, both grad scales and weight decays, the four EMA
    modes; max_norm brackets the norm as ADAM_CASES says; the update is resolved in fp32 p; fp32 torch is under BAR_A / 4."""
    cs = er.ADAM_CASES
    assert {c[0] for c in cs} == set(er.ADAM_STEPS) and {c[1] for c in cs} == {0.0, 0.05, 10.0} and {c[2] for c in cs} == {1.0, 0.125}
    assert {c[3] for c in cs} == {0.0, 1e-2} and {c[4] for c in cs} == {"none", None, 0.0, 0.9996}
    d = er.adam_data(er.ADAM_N)
    assert 0.04 < float(d["p"].abs().mean()) < 0.06 and float(d["v"].min()) > 0 and float((d["ema"] - d["p"]).abs().min()) >= 0
    assert float(d["m"].abs().min()) > 0 and not torch.equal(d["ema"], d["p"])
    for c in cs:
        ref = er.adam_ref(d, c)
        nrm = float(ref["norm"][0])
        assert 0.05 < nrm < 10.0, nrm
        upd = (ref["p"][0] - d["p"].double() * (1 - er.ADAM_LR * c[3])).abs()
        assert float(upd.mean()) > 100 * 2.0 ** -24 * 0.1, "the update must be well above ulp(p)"
        e32_ok(ref, er.adam_ref(d, c, torch.float32), f"adamw {c}")
    dw = er.adam_data(er.WRAP_ADAMW)
    assert dw["p"].numel() == er.WRAP_ADAMW and float(torch.linalg.vector_norm(dw["g"].double())) > er.ADAM_WRAP_CASE[1]


def test_sumsq_reference():
    g = er.data((er.ADAM_N + 1,), "sumsq.g", 0.02)
    r = er.sumsq(g)
    near(r["sumsq"][0], torch.linalg.vector_norm(g.double()) ** 2)
    e32_ok(r, er.sumsq(g, torch.float32), "sumsq")
    g = torch.full((er.ADAM_N + 1,), 1e-4)
    g[-1] = 1e3
    e32_ok(er.sumsq(g), er.sumsq(g, torch.float32), "sumsq spike")


def test_wrap_sizes():
    """Each wrap size gives its kernel's threads a second, partial and ragged trip; nothing needs more than about 200 MB."""
    cap = er.CAP_THREADS
    for n, k in ((er.WRAP_1, 1), (3 * er.WRAP_B3, 1), (er.WRAP_ADAMW, 4), (er.WRAP_SUMSQ, 16), (er.WRAP_X4, 1)):
        assert min((n // k + 255) // 256, 8192) == 8192 and cap * k < n < cap * k + 256 * k * 4 and n % 4
    assert er.wrap_size(1, True) % 4 == 0 and 3 * er.WRAP_B3 - er.WRAP_1 < 6 and er.WRAP_SUMSQ * 4 < 200e6
    assert (3 * er.RAGGED_N) % 4 and (3 * er.RAGGED_N) % 64 and er.RAGGED_N % 64
    t = er.data((2 * er._BLOCK + 5,), "tile", 1.0)
    assert torch.equal(t[:er._BLOCK], t[er._BLOCK:2 * er._BLOCK]) and torch.equal(t[:5], t[2 * er._BLOCK:])


# ------------------------------------------------------------------------------------------------ the movers
def test_layout_references_match_torch():
    B, C, H, W = 3, 3, 5, 7
    x = er.data((B, C, H, W), "l.x", 1.0, _f64)
    mul = er.data((B,), "coef.mul", 0.5, _f64) + 1.5
    for cpad in (3, 4, 32):
        y = er.nchw_to_nhwc(x, mul, cpad)["y"][0]
        near(y[..., :C], (x * mul.reshape(B, 1, 1, 1)).permute(0, 2, 3, 1))
        assert y.shape == (B, H, W, cpad) and float(y[..., C:].abs().sum()) == 0
        f = er.data((B, H, W, cpad), "p.f", 1.3, _f64)
        out = er.precond_out(x, f, mul, mul[:1] * 2, C)["out"][0]
        near(out, mul.reshape(B, 1, 1, 1) * x + mul[0] * 2 * f[..., :C].permute(0, 3, 1, 2))
        # the adjoints: <precond_out(None, f, s), dout> == <f, precond_out_bwd(dout, s)>
        dout = er.data((B, C, H, W), "p.dout", 1.0, _f64)
        lhs = (er.precond_out(None, f, None, mul, C)["out"][0] * dout).sum()
        rhs = (f * er.precond_out_bwd(dout, mul, cpad)["df"][0]).sum()
        near(lhs, rhs, 1e-12)
    yv, xv = er.data((B, 50), "ax.y", 1.0, _f64), er.data((B, 50), "ax.x", 1.0, _f64)
    near(er.axpby_b(xv, yv, mul, mul[:1])["out"][0], mul[0] * yv + mul.reshape(B, 1) * xv)
    near(er.axpby_b(None, yv, None, mul)["out"][0], mul.reshape(B, 1) * yv)


def test_mover_references_match_torch():
    x = er.data((3, 6, 10, 36), "r.x", 1.0, _f64)
    nchw = x.permute(0, 3, 1, 2)
    near(er.resample2x(x, 0, 0.25)["y"][0], F.avg_pool2d(nchw, 2).permute(0, 2, 3, 1))
    near(er.resample2x(x, 0, 1.0)["y"][0], 4 * F.avg_pool2d(nchw, 2).permute(0, 2, 3, 1))
    up = F.interpolate(nchw, scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(er.resample2x(x, 1, 1.0)["y"][0], up)
    pre = er.data(tuple(up.shape), "r.pre", 1.0, _f64)
    near(er.resample2x(x, 1, 0.25, pre)["y"][0], 0.25 * up + pre)
    a, b = er.data((107, 36), "c.a", 1.0, _f64), er.data((107, 4), "c.b", 1.3, _f64)
    assert torch.equal(er.concat2(a, b, 1.0)["y"][0], torch.cat([a, b], dim=1))
    near(er.concat2(a, b, 0.7)["y"][0], torch.cat([a, 0.7 * b], dim=1))
    dy = er.data((107, 40), "c.dy", 1.0, _f64)
    s = er.split2(dy, 36, 0.7)
    near((er.concat2(a, b, 0.7)["y"][0] * dy).sum(), (a * s["da"][0]).sum() + (b * s["db"][0]).sum(), 1e-12)
    src, dst = er.data((107, 20), "cc.src", 1.0, _f64), er.data((107, 16), "cc.dst", 1.3, _f64)
    for acc in (0, 1):
        r, m = er.copy_channels(src, 8, dst, 4, 8, 0.37, acc)["dst"]
        want = dst.clone()
        want[:, 4:12] = 0.37 * src[:, 8:16] + (dst[:, 4:12] if acc else 0)
        near(r, want)
        assert bool((m >= r.abs() * (1 - 1e-12)).all())
    near(er.add(a, a * 2, a * 3)["y"][0], 6 * a), near(er.add(a, a * 2)["y"][0], 3 * a)


def test_silu_and_embedding_references():
    x = er.data((3027,), "a.x", 12.0, _f64)
    x[:4] = torch.tensor([-100.0, 100.0, -88.0, 88.0], dtype=_f64)
    xg = x.clone().requires_grad_(True)
    dy = er.data((3027,), "a.b", 1.3, _f64)
    r = er.silu(x, dy)
    (gx,) = torch.autograd.grad(F.silu(xg), xg, dy)
    near(r["y"][0], F.silu(x)), near(r["dx"][0], gx)
    e32_ok(r, er.silu(x, dy, torch.float32), "silu")
    for C in (2, 192):
        t = torch.tensor([math.log(1e-4), -1.0, 0.0], dtype=torch.float32)
        r = er.pos_embedding(t, C)
        half = C // 2
        fr = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=_f64) / half)
        near(r["emb"][0], torch.cat([torch.cos(t.double()[:, None] * fr), torch.sin(t.double()[:, None] * fr)], dim=1), 1e-12)
        e32_ok(r, er.pos_embedding(t, C, torch.float32), f"pos_embedding {C}")


def test_fp32_baseline_of_the_movers_is_under_the_ceiling():
    B, C, H, W = 3, 3, 5, 7
    x, f = er.data((B, C, H, W), "p.x", 1.0), er.data((B, H, W, 4), "p.f", 1.3)
    a, s = er.data((B,), "coef.a", 0.5) + 1.5, er.data((B,), "coef.s", 0.5) + 1.5
    xr = er.data((3, 6, 10, 4), "r.x", 1.0)
    ca, cb = er.data((107, 36), "c.a", 1.0), er.data((107, 4), "c.b", 1.3)
    for name, fn, args in (("nchw_to_nhwc", er.nchw_to_nhwc, (x, a, 4)), ("precond_out", er.precond_out, (x, f, a, s, C)),
                           ("precond_out_bwd", er.precond_out_bwd, (x, s, 4)), ("axpby_b", er.axpby_b, (x.reshape(B, -1), x.reshape(B, -1) * 2, a, s)),
                           ("resample down", er.resample2x, (xr, 0, 0.25, None)), ("resample up acc", er.resample2x, (xr, 1, 0.25, er.data((3, 12, 20, 4), "r.pre", 1.0))),
                           ("concat2", er.concat2, (ca, cb, er.f32(0.7071067811865476))), ("split2", er.split2, (ca, 8, er.f32(0.7071067811865476))),
                           ("add3", er.add, (ca, ca * 1.3, ca * 0.7))):
        e32_ok(fn(*args), fn(*args, torch.float32), name)
