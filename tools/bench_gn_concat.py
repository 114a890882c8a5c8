#!/usr/bin/env python3
"""Decoder-block input, C ABI timing at the bench's decoder shapes (bs 128): the two-step path (adm_concat2 + adm_gn_fwd_amax;
adm_gn_bwd_add_amax + adm_split2) against the concat forms of the GroupNorm kernels (adm_gn_fwd_cat_amax, adm_gn_bwd_add_cat_amax).
With a library that does not export the concat forms only the two-step columns are printed (diagnostic; GPU box)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adm_amd import hip, ops  # noqa: E402
from adm_amd.hip import call, ptr  # noqa: E402

B = 128
dev = torch.device("cuda:0")
lib = hip.lib()
HAVE_CAT = "adm_gn_fwd_cat_amax" in hip.EXPORTS


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3          # us


print(f"{'shape':>22s}  {'concat2+fwd':>12s} {'fwd_cat':>9s} {'saved':>7s}   {'bwd+split2':>11s} {'bwd_cat':>9s} {'saved':>7s}   (us; GB/s of the bytes the result needs)")
for h, ca, cb in [(32, 384, 192), (32, 192, 192), (16, 384, 384), (8, 384, 384)]:
    C, HW, M = ca + cb, h * h, B * h * h
    G = min(32, C // 4)
    S = lib.adm_gn_splits(HW, C)
    f32 = dict(device=dev, dtype=torch.float32)
    a, b = torch.randn(B, h, h, ca, **f32), torch.randn(B, h, h, cb, **f32)
    gam, bet = torch.randn(C, **f32), torch.randn(C, **f32)
    dy, add = torch.randn(B, h, h, C, **f32), torch.randn(B, h, h, C, **f32)
    z, y, dz = (torch.empty(B, h, h, C, **f32) for _ in range(3))
    da, db = torch.empty(B, h, h, ca, **f32), torch.empty(B, h, h, cb, **f32)
    stats = torch.empty(B, G, 2, **f32)
    ws = torch.empty(B * S * G * 2, device=dev, dtype=torch.float64)
    red = torch.empty(B * S * C * 2 + B * C * 2 + B * G * 2, **f32)
    bz, by, bd = (torch.zeros(ops.AMAX_FLOATS, **f32) for _ in range(3))

    def fwd2():
        call("adm_concat2", ptr(a), ca, ptr(b), cb, ptr(z), M, 1.0, ptr(bz))
        call("adm_gn_fwd_amax", ptr(z), ptr(stats), ptr(ws), ptr(gam), ptr(bet), None, 0, ptr(y), ptr(by), B, HW, C, G, 1e-5, 1, 0.0, 0)

    def bwd2():
        call("adm_gn_bwd_add_amax", ptr(z), ptr(dy), ptr(stats), ptr(gam), ptr(bet), None, 0, ptr(add), ptr(dz), None, None, None, ptr(red),
             ptr(bd), B, HW, C, G, 1, 0.0, 0)
        call("adm_split2", ptr(dz), ptr(da), ca, ptr(db), cb, M, 1.0)

    def fwd1():
        call("adm_gn_fwd_cat_amax", ptr(a), ca, ptr(b), cb, 1.0, ptr(z), ptr(bz), ptr(stats), ptr(ws), ptr(gam), ptr(bet), None, 0, ptr(y),
             ptr(by), B, HW, G, 1e-5, 1, 0.0, 0)

    def bwd1():
        call("adm_gn_bwd_add_cat_amax", ptr(z), ptr(dy), ptr(stats), ptr(gam), ptr(bet), None, 0, ptr(add), ptr(da), ca, ptr(db), cb, 1.0, None,
             None, None, ptr(red), ptr(bd), B, HW, G, 1, 0.0, 0)

    n = 4.0 * M * C
    tf2, tb2 = timeit(fwd2), timeit(bwd2)
    line = f"{h:2d}x{h:<2d} {C:4d} = {ca:3d} + {cb:3d}  {tf2:12.1f}"
    if HAVE_CAT:
        tf1, tb1 = timeit(fwd1), timeit(bwd1)
        # needed forward: read a | b, write z, write y (3 passes); backward: read z, dy, addend, write da | db (4 passes)
        line += f" {tf1:9.1f} {tf2 - tf1:7.1f}   {tb2:11.1f} {tb1:9.1f} {tb2 - tb1:7.1f}   fwd {3 * n / tf1 / 1e3:5.0f}, bwd {4 * n / tb1 / 1e3:5.0f} GB/s"
    else:
        line += f" {'-':>9s} {'-':>7s}   {tb2:11.1f} {'-':>9s} {'-':>7s}"
    print(line, flush=True)
