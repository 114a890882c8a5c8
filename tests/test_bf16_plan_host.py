"""CPU-only: the launch plans of the direct bf16 kernels as host queries, and the conditioning of the sweep's data.

adm_conv_bf16_tile / adm_conv_wgrad_bf16_plan are the functions the launchers of conv_igemm_bf16.hip / conv_wgrad_bf16.hip call, so
what they answer is what runs.  This file pins them for every geometry of tests/test_hip_bf16_accuracy.py (so "the atomic path ran"
and "the 128x96 form ran" are facts of the table, not assumptions), records which forward forms the CIFAR UNet of BASELINE configs[2]
reaches at its per-GPU batch, and checks that on the sweep's data an honest fp32 accumulation of the bf16-rounded operands is inside
bar A of tests/test_hip_accuracy.py -- the bar the kernels are then held to on the GPU.
"""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import bf16_cases as bc
import fp64ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_A = 1e-5
QUERIES = ("adm_conv_bf16_tile", "adm_conv_wgrad_bf16_plan")


def _lib():
    from adm_amd import hip
    return hip.lib()


def test_queries_are_declared_and_exported():
    from adm_amd import hip
    header = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    lib = _lib()
    for name in QUERIES:
        assert re.search(r"^int\s+%s\s*\(" % name, header, flags=re.M), name
        assert name in hip.EXPORTS and name in hip.NO_STREAM and hasattr(lib, name)
    out = (ctypes.c_int * 4)()
    assert lib.adm_conv_bf16_tile(0, 64) == -22 and lib.adm_conv_bf16_tile(64, 0) == -22
    assert lib.adm_conv_wgrad_bf16_plan(64, 64, 64, 3, 1, None) == -22          # no output
    assert lib.adm_conv_wgrad_bf16_plan(64, 48, 64, 3, 1, out) == -22            # what the launcher refuses: Cin % 32, Cout % 32, ks
    assert lib.adm_conv_wgrad_bf16_plan(64, 64, 48, 3, 1, out) == -22
    assert lib.adm_conv_wgrad_bf16_plan(64, 64, 64, 2, 1, out) == -22
    assert lib.adm_conv_wgrad_bf16_plan(0, 64, 64, 3, 1, out) == -22


def test_forward_heuristic_on_the_sweep_geometries():
    """Every sweep geometry fits one round of slots, where the 64x64 form is cheapest (20480 against 25869 and 32768): the heuristic
    alone would never run the other two forms at test size, which is why the sweep forces `tile`."""
    lib = _lib()
    for g in bc.FWD:
        assert lib.adm_conv_bf16_tile(g[0] * g[1] * g[2], g[4]) == 2, g
    # the example of the issue: M = 131072, N = 192 -> 128x96 (4 waves along M, three 32-column blocks per wave)
    assert lib.adm_conv_bf16_tile(131072, 192) == 1


def test_every_form_meets_both_epilogues_in_the_sweep():
    """Each of the three forms runs its unguarded (`full`) and its guarded epilogue somewhere in the sweep -- once both in one launch, once
    each alone -- and meets an exact grid, a grid that is ragged in both M and N, and one that is ragged in one of them only."""
    for tile, (BM, BN) in bc.TILES.items():
        eps = [bc.epilogues(g, tile) for g in bc.FWD]
        assert any(f and r for f, r in eps) and any(f and not r for f, r in eps) and any(r and not f for f, r in eps), (tile, eps)
        ragged = {((g[0] * g[1] * g[2]) % BM != 0, g[4] % BN != 0) for g in bc.FWD}
        assert (True, True) in ragged and (False, False) in ragged and len(ragged) >= 3, (tile, ragged)


@pytest.mark.parametrize("key", list(bc.WGRAD_PLANS), ids=lambda k: f"{bc.geom_id(k[0])}-s{k[1]}")
def test_wgrad_plan_table(key):
    g, splits = key
    B, H, W, ci, co, ks, up = g
    out = (ctypes.c_int * 4)()
    assert _lib().adm_conv_wgrad_bf16_plan(B * H * W, ci, co, ks, splits, out) == 0
    assert tuple(out) + (bc.is_fast(g),) == bc.WGRAD_PLANS[key]
    TM, TN, s, chunk = tuple(out)
    assert chunk % 64 == 0 and (s - 1) * chunk < B * H * W <= s * chunk          # every split but the last is whole; none is empty


def test_wgrad_sweep_reaches_every_form():
    """The table holds all four tile forms on both load paths' side of the FAST rule, plain stores, the explicit atomic split (with a
    short last chunk) and both automatic modes as atomic two-way splits."""
    plans = bc.WGRAD_PLANS
    assert {p[:2] for p in plans.values()} == {(64, 64), (64, 128), (128, 64), (128, 128)}
    assert {p[4] for (g, s), p in plans.items() if s == 1} == {True, False}
    for fast in (True, False):
        assert any(p[2] > 1 and p[4] == fast for (g, s), p in plans.items() if s > 1), fast
    for g in bc.WGRAD_SPLIT:
        P = g[0] * g[1] * g[2]
        assert all(plans[(g, s)][2] > 1 for s in (2, 3)), g                        # atomic
        assert any(P % plans[(g, s)][3] != 0 for s in (2, 3)), g                   # ... with a last chunk shorter than the others
    assert plans[(bc.WGRAD_AUTO, 0)][2] == 2 and plans[(bc.WGRAD_AUTO, -1)][2] == 2
    assert all((g, 1) in plans for g in bc.WGRAD) and all((g, s) in plans for g in bc.WGRAD_SPLIT for s in (2, 3))


# the forms configs[2] reaches: M = 128 H^2 down the table, N across
PRODUCTION_FORMS = {
    131072: {32: 2, 192: 1, 384: 0, 576: 1, 768: 0, 1152: 0},
    32768: {32: 2, 192: 1, 384: 1, 576: 1, 768: 0, 1152: 1},
    8192: {32: 2, 192: 2, 384: 2, 576: 1, 768: 1, 1152: 1},
    2048: {32: 2, 192: 2, 384: 2, 576: 2, 768: 2, 1152: 2},
}


def test_production_forms_of_the_cifar_unet():
    """The forward form per (M, N) of the CIFAR UNet at batch 128, with the widths derived from the model's parameter shapes: production
    reaches all three forms, and the GPU sweep forces each of them at every geometry."""
    lib = _lib()
    shapes = bc.production_shapes()
    assert sorted({n for _, n in shapes}) == [32, 192, 384, 576, 768, 1152]
    got = {}
    for M, N in shapes:
        got.setdefault(M, {})[N] = lib.adm_conv_bf16_tile(M, N)
    assert got == PRODUCTION_FORMS
    reached = {f for row in got.values() for f in row.values()}
    print("forms configs[2] reaches:", sorted(reached))
    assert reached == {0, 1, 2}
    assert reached <= set(bc.TILES)                                                  # test_hip_bf16_accuracy.py runs tile in bc.TILES


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _torch_f32(g, d):
    """Plain fp32 torch conv (and autograd's gradients) of a geometry on the operands rounded as the kernels round them: y from (x, w)
    with the fp32 bias and residual; dx from (dy, w); dw from (dy, x).  NHWC / OIHW results."""
    B, H, W, ci, co, ks, up = g
    r = bc.r16

    def run(x, w, dy, bias=None, res=None):
        x, w = _nchw(x).requires_grad_(True), w.clone().requires_grad_(True)
        xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
        y = F.conv2d(xin, w, bias, padding=ks // 2)
        if res is not None:
            y = y + _nchw(res)
        dx, dw = torch.autograd.grad(y, (x, w), _nchw(dy))
        return y.detach().permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1), dw

    y = run(r(d["x"]), r(d["w"]), d["dy"], d["bias"], d["res"])[0]
    dx = run(d["x"], r(d["w"]), r(d["dy"]))[1]
    dw = run(r(d["x"]), d["w"], r(d["dy"]))[2]
    return dict(y=y, dx=dx, dw=dw)


@pytest.mark.parametrize("g", sorted(set(bc.FWD + bc.WGRAD + [bc.WGRAD_AUTO])), ids=bc.geom_id)
def test_fp32_accumulation_is_inside_bar_a_on_the_sweep_data(g):
    """Reference conditioning: an honest fp32 accumulation of the rounded operands passes the bar the kernels are held to."""
    got, ref = _torch_f32(g, bc.data(g)), bc.references(g)
    for out in ("y", "dx", "dw"):
        e = fp64ref.errors(got[out], *ref[out])
        print(f"{bc.geom_id(g)} {out}: e_max {e[0]:.2e} e_rms {e[1]:.2e}")
        assert e[0] <= BAR_A, (out, e)
        assert float(ref[out][1].max()) > 0
