"""GPU: every GroupNorm (+ scale/shift + SiLU + dropout) launch plan against fp64, forward and backward.

Which kernels run depends on the shape: three register-resident one-launch templates (MAXR 2 / 8 / 14) with slabs of whole groups
for maps up to 16x16, the multi-pass kernels (moments -> finalize -> apply; partial -> reduce -> param -> dx) above that or where no
slab fits, split by the 64-row or the 256-row rule.  Every row of gn_cases.GRID is one test: it first asserts, through the host
query adm_gn_plan, that the row reaches the plan written next to it (a planner change fails here until the grid follows), then runs
ops.group_norm_act / group_norm_act_fork over its variants and data kinds -- on a one-launch row once more with adm_gn_fused(0), which
puts the multi-pass kernels on small maps -- and compares every output with fp64ref.group_norm.

Bar, per output and relative to the scale of fp64ref.group_norm's mag (fp64ref.errors): e_max <= BAR_A, the bar of the convs and
attention (tests/test_hip_accuracy.py).  On the offset data (|mean| / std = 15) the limit is max(BAR_A, 2 x the e_max of the fp32 torch
composition on the same data): the factor 2 of bar B.  tests/test_fp64ref_host.py shows on the CPU that plain fp32 arithmetic stays a
factor 4 below the bar on all of this data; a kernel that drops one pixel row from the moments of a 33x33 map is 30x above it.

Dropout: the mask is recovered from y (a dropped element is 0 where the undropped output is not).  dx is NOT zero where y was dropped
-- every element of a group receives the group-mean terms -- so the exact check is made where it holds: a dy that is non-zero ONLY at
dropped elements gives du = 0 everywhere, hence dx, dgamma and dbeta exactly 0.
"""
import ctypes
import math

import pytest
import torch

import fp64ref
import gn_cases
from test_hip_accuracy import BAR_A

pytestmark = pytest.mark.gpu

DROP_P, SEED = 0.1, 20240611
WORST = {}          # (plan, output) -> [e_max, e_rms]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip, ops as _ops
    hip.lib()        # raises if the HIP library is missing: no fallback
    return _ops


@pytest.fixture(autouse=True)
def _fp16_format_on(monkeypatch):
    """The switches these tests depend on, whatever the environment says: the fp16 format (so that GroupNorm writes bounds) and the
    end-of-backward parameter-gradient table."""
    from adm_amd import ops as _ops
    for name, v in (("COMPUTE", "f32"), ("FP16X3", True), ("BF16X6", True), ("DEFER_UNPACK", True), ("DETERMINISTIC", False)):
        monkeypatch.setattr(_ops, name, v)


def _lib():
    from adm_amd import hip
    return hip.lib()


def _plan(HW, C, G):
    out = (ctypes.c_int * 5)()
    assert _lib().adm_gn_plan(HW, C, G, out) == 0
    return tuple(out)


def _label(plan, forced):
    return "multi-pass, adm_gn_fused(0)" if forced else (f"one launch, MAXR {plan[3]}" if plan[0] else "multi-pass")


def _note(label, out, e):
    w = WORST.setdefault((label, out), [0.0, 0.0])
    w[0], w[1] = max(w[0], e[0]), max(w[1], e[1])


def _run(ops, row, c, *, silu, ss_mode, fork=False, drop_p=0.0, bound=False, backward=True, dy=None):
    """One op-level call (and its backward) on the GPU.  ss_mode: None, "full" [B, 2C], "bcast" [1, 2C], "slice" (columns
    32 .. 32 + 2C of a [B, 2C + 64] buffer, read in place).  Returns y, dx, dgamma, dbeta, dss and, with bound=True, the maxima of
    the bound vectors left on y and on dx."""
    H, W, C, groups, eps, B, _ = row
    dev = lambda t: t.cuda().contiguous()
    x, gam, bet = (dev(c[k]).requires_grad_(backward) for k in ("x", "gamma", "beta"))
    ss = None
    if ss_mode == "full":
        ss = dev(c["ss"]).requires_grad_(backward)
    elif ss_mode == "bcast":
        ss = dev(c["ss"][:1])
    elif ss_mode == "slice":
        pad = torch.full((B, 32), 1e3)                       # (read by mistake, it would not go unnoticed)
        ss = dev(torch.cat([pad, c["ss"], pad], dim=1))[:, 32:32 + 2 * C]
        assert ss.stride(0) == 2 * C + 64 and (B == 1 or not ss.is_contiguous())
    else:
        assert ss_mode is None
    seen = {}
    if backward:
        def hook(g):                 # inside the backward pass: the bound registered for dx is still this pass's
            v = ops._get_amax(g)
            seen["bound_dx"] = None if v is None else float(v.max())
        x.register_hook(hook)
    kw = dict(silu=silu, drop_p=drop_p, seed=SEED, groups=groups, eps=eps, to_conv=bound)
    if fork:
        y, xo = ops.group_norm_act_fork(x, gam, bet, ss, **kw)
    else:
        y = ops.group_norm_act(x, gam, bet, ss, **kw)
    got = {"y": y.detach()}
    if bound:
        assert hasattr(y, "_adm_amax") and y._adm_amax.numel() == ops.AMAX_FLOATS, "no bound vector on y"
        got["bound_y"] = float(y._adm_amax.max())
    else:
        assert not hasattr(y, "_adm_amax")
    if backward:
        dyd = dev(c["dy"] if dy is None else dy)
        if fork:
            torch.autograd.backward([y, xo], [dyd, dev(c["addend"])])      # the residual gradient enters the kernel as `addend`
        else:
            y.backward(dyd)
        got.update(dx=x.grad, dgamma=gam.grad, dbeta=bet.grad, bound_dx=seen.get("bound_dx"))
        if ss_mode == "full":
            got["dss"] = ss.grad
    return got


def _reference(row, c, *, silu, ss_mode, fork, keep=None, backward=True):
    G = gn_cases.groups_of(row)
    ss = {None: None, "full": c["ss"], "bcast": c["ss"][:1], "slice": c["ss"]}[ss_mode]
    kw = dict(groups=G, eps=row[4], silu=silu, keep=keep, addend=c["addend"] if fork else None, dy=c["dy"] if backward else None)
    return ss, kw, fp64ref.group_norm(c["x"].cuda(), c["gamma"], c["beta"], ss, **kw)


def _compare(where, label, got, ref, e32):
    """Every output of ref against the bar; e32 = the fp32 torch composition's e_max per output (offset data) or None."""
    line = []
    for n, (r, mag) in ref.items():
        e = fp64ref.errors(got[n], r, mag)
        _note(label, n, e)
        lim = BAR_A if e32 is None else max(BAR_A, 2.0 * e32[n])
        line.append(f"{n} {e[0]:.2e}" + ("" if e32 is None else f" (fp32 torch {e32[n]:.2e})"))
        assert e[0] <= lim, (where, label, n, e, lim)
    if e32 is not None:
        print(f"  {where} [{label}]: " + ", ".join(line))


def _bounds_are_exact(where, label, got, backward):
    assert got["bound_y"] == float(got["y"].abs().max()), (where, label, "y", got["bound_y"], float(got["y"].abs().max()))
    if backward:
        assert got["bound_dx"] is not None, (where, label, "no bound registered for dx")
        assert got["bound_dx"] == float(got["dx"].abs().max()), (where, label, "dx", got["bound_dx"], float(got["dx"].abs().max()))


# (name, silu, scale/shift, fork, backward, bound)
VARIANTS = [
    ("silu ss fork", True, "full", True, True, True),
    ("linear", False, None, False, True, False),
    ("silu", True, None, False, True, True),
    ("linear ss fork", False, "full", True, True, True),
    ("silu ss-broadcast", True, "bcast", False, False, True),
    ("linear ss-slice", False, "slice", False, False, False),
]


@pytest.mark.parametrize("row", gn_cases.GRID, ids=gn_cases.row_id)
def test_group_norm_plan_against_fp64(ops, row):
    H, W, C, _, eps, B, want = row
    HW, G = H * W, gn_cases.groups_of(row)
    cpg = C // G
    lib = _lib()
    assert ops._fp16_format()
    assert lib.adm_gn_fused(-1) == 1, "the one-launch kernels are switched off"
    assert _plan(HW, C, G) == want, "the planner no longer takes this row where the grid says: update gn_cases.GRID"
    if not want[0]:
        assert lib.adm_gn_splits(HW, C) == want[4]
    passes = [False, True] if want[0] else [False]           # one-launch rows: once more on the multi-pass kernels

    def each_plan(fn):
        """fn(forced, label) under the default plan and, on a one-launch row, under adm_gn_fused(0)."""
        res = []
        for forced in passes:
            if forced:
                assert lib.adm_gn_fused(0) == 1
            try:
                if forced:
                    assert _plan(HW, C, G)[0] == 0
                res.append(fn(forced, _label(want, forced)))
            finally:
                if forced:
                    lib.adm_gn_fused(1)
        return res

    for kind in gn_cases.KINDS:
        c = gn_cases.make_case(row, kind)
        for name, silu, ss_mode, fork, backward, bound in VARIANTS:
            where = f"{gn_cases.row_id(row)} {kind} {name}"
            ss, kw, ref = _reference(row, c, silu=silu, ss_mode=ss_mode, fork=fork, backward=backward)
            e32 = None
            if kind == "offset":
                t32 = gn_cases.torch_composition(c["x"], c["gamma"], c["beta"], ss, **kw)
                e32 = {n: fp64ref.errors(t32[n], *ref[n])[0] for n in ref}

            def one(forced, label):
                got = _run(ops, row, c, silu=silu, ss_mode=ss_mode, fork=fork, bound=bound, backward=backward)
                assert set(ref) <= set(got), (where, sorted(ref), sorted(got))
                _compare(where, label, got, ref, e32)
                if bound:
                    _bounds_are_exact(where, label, got, backward)
                if kind == "zero":
                    # variance 0: rstd = eps^-1/2, xhat = 0, so y is the affine offset -- the same value at every pixel -- and dx is finite
                    y0 = got["y"][0, :, :, :cpg]
                    assert torch.equal(y0, y0[:1, :1].expand_as(y0)), (where, label)
                    assert bool(torch.isfinite(got["y"]).all()), (where, label)
                    if backward:
                        assert bool(torch.isfinite(got["dx"]).all()), (where, label)
            each_plan(one)

        # ---- dropout: the mask comes back from y, the backward uses the same one, and so do both plans
        where = f"{gn_cases.row_id(row)} {kind} dropout"

        def forward_mask(forced, label):
            y0 = _run(ops, row, c, silu=True, ss_mode="full", backward=False)["y"]
            got = _run(ops, row, c, silu=True, ss_mode="full", fork=True, drop_p=DROP_P, bound=True)
            kept = (got["y"] != 0) | (y0 == 0)
            n = kept.numel()
            if n >= 2048:
                frac = 1.0 - float(kept.float().mean())
                assert abs(frac - DROP_P) <= 6.0 * math.sqrt(DROP_P * (1 - DROP_P) / n), (where, label, frac)
            return got, kept
        runs = each_plan(forward_mask)
        kept = runs[0][1]
        ref = None
        for forced, (got, k) in zip(passes, runs):
            if ref is None or not torch.equal(k, kept):          # the reference with the mask THIS plan's forward applied
                keep = k.double() / (1.0 - DROP_P)
                ss, kw, ref = _reference(row, c, silu=True, ss_mode="full", fork=True, keep=keep)
                e32 = None
                if kind == "offset":
                    t32 = gn_cases.torch_composition(c["x"], c["gamma"], c["beta"], ss, **dict(kw, keep=keep.float().cpu()))
                    e32 = {n: fp64ref.errors(t32[n], *ref[n])[0] for n in ref}
            _compare(where, _label(want, forced), got, ref, e32)
            _bounds_are_exact(where, _label(want, forced), got, True)
        for _, k in runs[1:]:
            assert torch.equal(k, kept), (where, "the two plans drop different elements")
        dy_dropped = c["dy"] * (~kept).float().cpu()             # a gradient that arrives only at dropped elements ...

        def only_dropped(forced, label):
            got = _run(ops, row, c, silu=True, ss_mode="full", drop_p=DROP_P, dy=dy_dropped)
            for n in ("dx", "dgamma", "dbeta", "dss"):           # ... goes nowhere: du = 0 everywhere, exactly
                assert int(torch.count_nonzero(got[n])) == 0, (where, label, n)
        each_plan(only_dropped)


def test_two_layers_share_one_parameter_gradient_launch(ops, monkeypatch):
    """Two GroupNorm layers of different width (16x16 / 32 and 8x8 / 384) in one backward pass, their gamma / beta accumulated
    directly: one adm_gn_bwd_param_table launch with two rows reduces both (its binary search finds the row of every block), and
    dgamma / dbeta agree with fp64.  One layer has a scale/shift, the other none (the table's null ss)."""
    rows = [next(r for r in gn_cases.GRID if r[:3] == k) for k in ((16, 16, 32), (8, 8, 384))]
    launches = []
    orig = ops.call

    def call(name, *args):
        if name == "adm_gn_bwd_param_table":
            launches.append(args[1:])
        return orig(name, *args)
    monkeypatch.setattr(ops, "call", call)
    ys, dys, params, refs = [], [], [], []
    for i, row in enumerate(rows):
        c = gn_cases.make_case(row, "plain")
        x = c["x"].cuda().requires_grad_(True)
        gam, bet = torch.nn.Parameter(c["gamma"].cuda()), torch.nn.Parameter(c["beta"].cuda())
        for p in (gam, bet):
            p.grad, p._adm_direct = torch.zeros_like(p), True
        ss = c["ss"].cuda() if i == 0 else None
        ys.append(ops.group_norm_act(x, gam, bet, ss, silu=True, groups=row[3], eps=row[4]))
        dys.append(c["dy"].cuda())
        params.append((gam, bet))
        refs.append(fp64ref.group_norm(c["x"].cuda(), c["gamma"], c["beta"], None if ss is None else c["ss"],
                                       groups=gn_cases.groups_of(row), eps=row[4], silu=True, dy=c["dy"]))
    torch.autograd.backward(ys, dys)
    torch.cuda.synchronize()
    assert launches == [(2, 1 + 12)], launches               # one launch, two rows, ceil(32 / 32) + ceil(384 / 32) blocks
    for row, (gam, bet), ref in zip(rows, params, refs):
        for n, p in (("dgamma", gam), ("dbeta", bet)):
            e = fp64ref.errors(p.grad, *ref[n])
            _note("parameter-gradient table", n, e)
            assert e[0] <= BAR_A, (gn_cases.row_id(row), n, e)


def test_grid_covers_every_plan_form():
    """The grid as a whole reaches every form of the launch plan (from the plans written in it, which the row tests assert)."""
    fused, multi = [], []
    for H, W, C, _, _, _, (Cc, threads, rows, maxr, S) in gn_cases.GRID:
        HW = H * W
        if Cc:
            R = threads // (Cc // 4)
            assert rows == -(-HW // R) and maxr in (2, 8, 14) and rows <= maxr
            fused.append(dict(maxr=maxr, tail=HW % R != 0, short=HW < R, threads=threads, edge=rows == maxr, slabs=C // Cc))
        else:
            R = threads // (C // 4)
            assert rows == -(-HW // S)
            multi.append(dict(uneven=HW % rows != 0, rule=64 if HW // 64 <= 16 else 256, R=R, threads=threads, HW=HW))
    for maxr in (2, 8, 14):
        for tail in (False, True):
            assert any(f["maxr"] == maxr and f["tail"] == tail for f in fused), (maxr, tail)
        assert any(f["maxr"] == maxr and f["edge"] for f in fused), maxr          # as many rows as the template holds
    assert any(f["short"] for f in fused)                                        # HW < R: whole thread-rows idle
    assert {240, 252} <= {f["threads"] for f in fused}                           # a partial last wave
    assert any(f["slabs"] > 1 for f in fused)
    assert any(m["uneven"] for m in multi)
    assert {64, 256} <= {m["rule"] for m in multi}
    assert any(m["R"] == 1 and m["threads"] > 256 for m in multi)
    assert any(m["HW"] <= 256 for m in multi)                                    # no slab fits
    assert any(m["threads"] < 256 and m["threads"] % 64 for m in multi)


def test_zz_report_worst_group_norm_errors():
    """Worst e_max / e_rms against fp64 per plan and output."""
    if not WORST:
        pytest.skip("no row ran in this session")
    print("\nGroupNorm: worst error vs fp64 per plan / output (e_max, e_rms):")
    for (label, out), (em, er) in sorted(WORST.items()):
        print(f"  {label:30s} {out:7s} {em:.3e} {er:.3e}")
