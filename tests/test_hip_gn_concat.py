"""GPU: the concat forms of the GroupNorm kernels (adm_gn_fwd_cat_amax / adm_gn_bwd_add_cat_amax, ops.group_norm_act_cat).

A decoder block's input is z = cat(a, scale_b * b) and its first op is norm0.fork(z).  The fused calls read the two halves in the
GroupNorm moments pass and write z as a side output; backward they write the two gradient halves in place of dz.  They promise the
SAME arithmetic in the same order as adm_concat2 + adm_gn_fwd_amax and adm_gn_bwd_add_amax + adm_split2, so the first check is bit
identity, not a tolerance: z, y, stats and both bounds forward; da, db, the per-image sums `tot` and the bound backward.  scale_b =
0.70710678 is the value that tells a contracted multiply-add from a rounded product (0.5 and 1.0 are exact either way).

Shapes (B = 3): the multi-pass kernels at 32x32 with (Ca, Cb) = (384, 192) -- C = 576, 18 channels per group, so groups straddle
the boundary -- and (192, 192); the three register-resident templates at 16x16 (MAXR 14), 8x8 (MAXR 8) and 4x4 (MAXR 2) with
(384, 384), where 48- and 96-channel slabs lie on either side of the boundary.

Against fp64 the bar is the one of tests/test_hip_groupnorm.py on its plain data: e_max <= BAR_A relative to fp64ref.group_norm's mag.
"""
import ctypes
import functools

import pytest
import torch

import fp64ref
from test_hip_accuracy import BAR_A

pytestmark = pytest.mark.gpu

B = 3
# (H, W, Ca, Cb, the plan adm_gn_plan must answer: MAXR, 0 = multi-pass)
SHAPES = [(32, 32, 384, 192, 0), (32, 32, 192, 192, 0), (16, 16, 384, 384, 14), (8, 8, 384, 384, 8), (4, 4, 384, 384, 2)]
SCALES = (1.0, 0.5, 0.70710678)
EPS = 1e-5
_id = lambda s: f"{s[0]}x{s[1]}-{s[2]}+{s[3]}"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip, ops as _ops
    hip.lib()        # raises if the HIP library is missing: no fallback
    return _ops


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    from adm_amd import ops as _ops
    for name, v in (("COMPUTE", "f32"), ("FP16X3", True), ("BF16X6", True), ("H3_GEMM", True), ("GN_CONCAT", True)):
        monkeypatch.setattr(_ops, name, v)


@functools.lru_cache(maxsize=8)
def make_case(shape):
    """CPU fp32 tensors of a shape; fixed generator.  Shared: do not modify."""
    H, W, ca, cb, _ = shape
    C = ca + cb
    gen = torch.Generator().manual_seed(1000 * H + ca + 7 * cb)
    rn = lambda *s: torch.randn(*s, generator=gen)
    ru = lambda *s: torch.rand(*s, generator=gen) * 2 - 1
    return dict(a=rn(B, H, W, ca) * 2.0 + 0.3, b=rn(B, H, W, cb) * 1.5 - 0.2, gamma=1.0 + 0.2 * ru(C), beta=0.1 * ru(C),
                dy=rn(B, H, W, C), addend=rn(B, H, W, C))


def _plan(HW, C, G):
    from adm_amd import hip
    out = (ctypes.c_int * 5)()
    assert hip.lib().adm_gn_plan(HW, C, G, out) == 0
    return tuple(out)


def _vec(ops, like):
    return torch.zeros(ops.AMAX_FLOATS, device=like.device, dtype=torch.float32)


def _two_step_and_fused(ops, shape, scale, with_add, with_bound):
    """Both paths at the C ABI on the same inputs; returns two dicts of everything either path leaves."""
    from adm_amd.hip import call, ptr, lib
    H, W, ca, cb, _ = shape
    C, HW, M = ca + cb, H * W, B * H * W
    G = min(32, C // 4)
    S = lib().adm_gn_splits(HW, C)
    c = {k: v.cuda() for k, v in make_case(shape).items()}
    f32 = dict(device="cuda", dtype=torch.float32)
    new = lambda *s: torch.full(s, float("nan"), **f32)           # (an element nobody writes does not compare equal)
    add = c["addend"] if with_add else None
    out = []
    for fused in (False, True):
        z, y, stats = new(B, H, W, C), new(B, H, W, C), new(B, G, 2)
        ws = torch.zeros(B * S * G * 2, device="cuda", dtype=torch.float64)
        bz, by, bd = (_vec(ops, z) if with_bound else None for _ in range(3))
        da, db = new(B, H, W, ca), new(B, H, W, cb)
        red = torch.zeros(B * S * C * 2 + B * C * 2 + B * G * 2, **f32)
        if fused:
            call("adm_gn_fwd_cat_amax", ptr(c["a"]), ca, ptr(c["b"]), cb, scale, ptr(z), ptr(bz), ptr(stats), ptr(ws), ptr(c["gamma"]),
                 ptr(c["beta"]), None, 0, ptr(y), ptr(by), B, HW, G, EPS, 1, 0.0, 0)
            call("adm_gn_bwd_add_cat_amax", ptr(z), ptr(c["dy"]), ptr(stats), ptr(c["gamma"]), ptr(c["beta"]), None, 0, ptr(add), ptr(da), ca,
                 ptr(db), cb, scale, None, None, None, ptr(red), ptr(bd), B, HW, G, 1, 0.0, 0)
        else:
            dz = new(B, H, W, C)
            call("adm_concat2", ptr(c["a"]), ca, ptr(c["b"]), cb, ptr(z), M, scale, ptr(bz))
            if with_bound:
                call("adm_gn_fwd_amax", ptr(z), ptr(stats), ptr(ws), ptr(c["gamma"]), ptr(c["beta"]), None, 0, ptr(y), ptr(by), B, HW, C, G,
                     EPS, 1, 0.0, 0)
                call("adm_gn_bwd_add_amax", ptr(z), ptr(c["dy"]), ptr(stats), ptr(c["gamma"]), ptr(c["beta"]), None, 0, ptr(add), ptr(dz), None,
                     None, None, ptr(red), ptr(bd), B, HW, C, G, 1, 0.0, 0)
            else:
                call("adm_gn_fwd", ptr(z), ptr(stats), ptr(ws), ptr(c["gamma"]), ptr(c["beta"]), None, 0, ptr(y), B, HW, C, G, EPS, 1, 0.0, 0)
                call("adm_gn_bwd_add", ptr(z), ptr(c["dy"]), ptr(stats), ptr(c["gamma"]), ptr(c["beta"]), None, 0, ptr(add), ptr(dz), None, None,
                     None, ptr(red), B, HW, C, G, 1, 0.0, 0)
            call("adm_split2", ptr(dz), ptr(da), ca, ptr(db), cb, M, scale)
        torch.cuda.synchronize()
        tot = red[B * S * C * 2:B * S * C * 2 + B * C * 2]
        res = dict(z=z, y=y, stats=stats, da=da, db=db, tot=tot.clone())
        if with_bound:
            res.update(bound_z=bz.max().reshape(1), bound_y=by.max().reshape(1), bound_dz=bd.max().reshape(1))
        out.append(res)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_fused_calls_are_bit_identical_to_the_two_step_path(ops, shape):
    H, W, ca, cb, maxr = shape
    C = ca + cb
    assert _plan(H * W, C, min(32, C // 4))[3] == maxr, "the planner no longer takes this shape where the test says"
    for scale in SCALES:
        for with_add in (False, True):
            for with_bound in (False, True):
                two, one = _two_step_and_fused(ops, shape, scale, with_add, with_bound)
                where = (_id(shape), scale, with_add, with_bound)
                assert set(two) == set(one)
                for k in two:
                    assert not bool(torch.isnan(two[k]).any()), (where, k, "the two-step path left elements unwritten")
                    assert torch.equal(two[k], one[k]), (where, k, float((two[k] - one[k]).abs().max()))
                if with_bound:       # ... and the bounds are the maxima of what was written (of dz before the scaling)
                    assert float(one["bound_z"]) == float(one["z"].abs().max()), where
                    assert float(one["bound_y"]) == float(one["y"].abs().max()), where
                    dmax = max(float(one["da"].abs().max()), float(one["db"].abs().max()))
                    assert float(one["bound_dz"]) >= dmax, where
                    if scale == 1.0:
                        assert float(one["bound_dz"]) == dmax, where
    # z is torch.cat of the halves, the second one scaled in fp32
    c = make_case(shape)
    one = _two_step_and_fused(ops, shape, SCALES[2], False, False)[1]
    assert torch.equal(one["z"].cpu(), torch.cat((c["a"], c["b"] * torch.tensor(SCALES[2])), dim=-1))


def _op_run(ops, shape, scale, with_add):
    """ops.group_norm_act_cat and its backward; returns y, z, da, db, dgamma, dbeta and the bounds the op left."""
    c = make_case(shape)
    a, b, gam, bet = (c[k].cuda().requires_grad_(True) for k in ("a", "b", "gamma", "beta"))
    seen = {}

    def hook(name):
        def h(g):                    # inside the backward pass: the bound registered for this gradient is still this pass's
            v = ops._get_amax(g)
            seen[name] = None if v is None else float(v.max())
        return h
    a.register_hook(hook("bound_da")); b.register_hook(hook("bound_db"))
    y, z = ops.group_norm_act_cat(a, b, scale, gam, bet, silu=True, to_conv=True)
    got = dict(y=y.detach(), z=z.detach(), bound_y=float(y._adm_amax.max()), bound_z=float(z._adm_amax.max()))
    if with_add:
        torch.autograd.backward([y, z], [c["dy"].cuda(), c["addend"].cuda()])
    else:
        y.backward(c["dy"].cuda())
    got.update(da=a.grad, db=b.grad, dgamma=gam.grad, dbeta=bet.grad, **seen)
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_group_norm_act_cat_against_fp64(ops, shape, monkeypatch):
    """The op (autograd Function included) against fp64ref.group_norm on z = cat(a, fp32(scale_b * b)); the fused op against its own
    two-step fallback (ADM_GN_CONCAT=0), bit for bit; the bounds it leaves and registers."""
    H, W, ca, cb, _ = shape
    C = ca + cb
    c = make_case(shape)
    calls = []
    orig = ops.call

    def call(name, *args):
        calls.append(name)
        return orig(name, *args)
    monkeypatch.setattr(ops, "call", call)
    for scale in SCALES:
        for with_add in (False, True):
            where = (_id(shape), scale, with_add)
            del calls[:]
            got = _op_run(ops, shape, scale, with_add)
            assert "adm_gn_fwd_cat_amax" in calls and "adm_gn_bwd_add_cat_amax" in calls and "adm_concat2" not in calls, (where, calls)
            z = torch.cat((c["a"], c["b"] * torch.tensor(scale)), dim=-1)
            assert torch.equal(got["z"].cpu(), z), where
            ref = fp64ref.group_norm(z.cuda(), c["gamma"], c["beta"], None, groups=min(32, C // 4), eps=EPS, silu=True,
                                     addend=c["addend"] if with_add else None, dy=c["dy"])
            dz, dz_mag = ref["dx"]
            parts = dict(y=ref["y"], dgamma=ref["dgamma"], dbeta=ref["dbeta"], da=(dz[..., :ca], dz_mag[..., :ca]),
                         db=(scale * dz[..., ca:], abs(scale) * dz_mag[..., ca:]))
            for n, (r, mag) in parts.items():
                e = fp64ref.errors(got[n], r, mag)
                print(f"  {where} {n}: e_max {e[0]:.2e} e_rms {e[1]:.2e}")
                assert e[0] <= BAR_A, (where, n, e)
            assert got["bound_y"] == float(got["y"].abs().max()) and got["bound_z"] == float(got["z"].abs().max()), where
            assert got["bound_da"] is not None and got["bound_da"] >= float(got["da"].abs().max()), where
            assert got["bound_db"] is not None and got["bound_db"] >= float(got["db"].abs().max()), where      # every scale here is <= 1
            monkeypatch.setattr(ops, "GN_CONCAT", False)
            del calls[:]
            two = _op_run(ops, shape, scale, with_add)
            monkeypatch.setattr(ops, "GN_CONCAT", True)
            assert "adm_concat2" in calls and "adm_gn_fwd_cat_amax" not in calls, (where, calls)
            for n in got:
                same = torch.equal(got[n], two[n]) if torch.is_tensor(got[n]) else got[n] == two[n]
                assert same, (where, n, "the fused op and its two-step fallback differ")


def test_a_scale_above_one_registers_no_bound_for_db(ops):
    """max |dz| bounds db = scale_b * dz[:, Ca:] only for |scale_b| <= 1: above, da keeps its bound and db gets none."""
    got = _op_run(ops, SHAPES[-1], 1.5, True)
    assert got["bound_da"] is not None and got["bound_db"] is None


def _training_step(ops, gpu, fused, monkeypatch):
    from test_hip_model import make_ddpm
    from oracle import fill
    monkeypatch.setattr(ops, "GN_CONCAT", fused)
    calls = []
    orig = ops.call

    def call(name, *args):
        calls.append(name)
        return orig(name, *args)
    monkeypatch.setattr(ops, "call", call)
    dpm, *_ = make_ddpm("const", gpu)
    dpm.train()
    x0 = fill.hash_tensor((2, 3, 32, 32), "x0", 1.0)
    noise = fill.hash_tensor((2, 3, 32, 32), "noise", 1.7)
    t = torch.tensor([0.23, 0.81])
    loss, _ = dpm.training_step({"image": x0.to(gpu)}, t=t.to(gpu), noise=noise.to(gpu))
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "call", orig)
    return loss.detach().clone(), {n: p.grad.clone() for n, p in dpm.named_parameters() if p.grad is not None}, calls


def test_training_step_is_bit_identical_with_and_without_the_fused_concat(ops, monkeypatch):
    """One training step of the reduced two-decoder UNet in deterministic mode, ADM_GN_CONCAT on and off: the loss and every parameter
    gradient agree bit for bit (every 3x3 layer forced onto the Winograd kernels, so the bounds decide formats as in the bench)."""
    gpu = torch.device("cuda:0")
    monkeypatch.setattr(ops, "DETERMINISTIC", True)
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    loss1, g1, calls1 = _training_step(ops, gpu, True, monkeypatch)
    loss0, g0, calls0 = _training_step(ops, gpu, False, monkeypatch)
    n_cat = calls0.count("adm_concat2")
    assert n_cat > 0 and calls0.count("adm_split2") == n_cat and "adm_gn_fwd_cat_amax" not in calls0
    assert calls1.count("adm_gn_fwd_cat_amax") == n_cat and calls1.count("adm_gn_bwd_add_cat_amax") == n_cat
    assert "adm_concat2" not in calls1 and "adm_split2" not in calls1
    assert torch.equal(loss1, loss0), (float(loss1), float(loss0))
    assert set(g1) == set(g0) and len(g1) > 400
    bad = [n for n in g0 if not torch.equal(g1[n], g0[n])]
    assert not bad, bad[:10]


def test_training_step_under_amax_check_with_the_fused_concat(ops, monkeypatch):
    """... and one step with every bound that reaches a consumer verified against the tensor it came with (ADM_AMAX_CHECK semantics)."""
    gpu = torch.device("cuda:0")
    monkeypatch.setattr(ops, "AMAX_CHECK", True)
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    loss, grads, calls = _training_step(ops, gpu, True, monkeypatch)
    assert calls.count("adm_gn_fwd_cat_amax") > 0 and bool(torch.isfinite(loss))
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
