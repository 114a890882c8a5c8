"""The GroupNorm launch-plan grid, its data and the fp32 torch composition, shared by tests/test_fp64ref_host.py (CPU) and
tests/test_hip_groupnorm.py (GPU).  A plain helper like parity.py, not a conftest.

A grid row is (H, W, C, groups, eps, B, plan); groups = 0 is the UNet's min(32, C // 4).  plan is what adm_gn_plan must answer for the
row under the default switch: (Cc, threads, rows, MAXR, S) -- Cc = 0 means the multi-pass kernels, `rows` is rows per thread on the
one-launch path and rows per split on the multi-pass path.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

GRID = [
    # ---- one launch, MAXR 2
    (1, 1, 32, 8, 1e-5, 2, (32, 256, 1, 2, 1)),          # HW < R (R = 32): one thread-row of 32 works
    (2, 2, 32, 8, 1e-5, 2, (32, 256, 1, 2, 1)),          # HW < R
    (8, 8, 32, 8, 1e-5, 2, (32, 256, 2, 2, 1)),          # rows 2 (template edge), no tail
    (4, 4, 192, 0, 1e-5, 2, (96, 240, 2, 2, 1)),         # 240 threads, R 10, tail
    (4, 4, 768, 0, 1e-5, 2, (96, 240, 2, 2, 1)),         # 8 slabs
    # ---- MAXR 8
    (5, 5, 96, 0, 1e-5, 2, (96, 240, 3, 8, 1)),          # G 24, tail
    (9, 7, 64, 32, 1e-5, 2, (64, 256, 4, 8, 1)),         # cpg 2, R 16, tail
    (8, 8, 384, 0, 1e-5, 2, (96, 240, 7, 8, 1)),         # tail
    (16, 16, 32, 8, 1e-5, 2, (32, 256, 8, 8, 1)),        # rows 8 (template edge), no tail
    (16, 16, 128, 32, 1e-6, 2, (32, 256, 8, 8, 1)),      # the autoencoder's groups / eps, 4 slabs
    # ---- MAXR 14
    (14, 10, 192, 0, 1e-5, 2, (96, 240, 14, 14, 1)),     # rows 14 (template edge), no tail
    (12, 11, 192, 0, 1e-5, 2, (96, 240, 14, 14, 1)),     # tail
    (16, 16, 36, 6, 1e-5, 2, (36, 252, 10, 14, 1)),      # cpg 6: quads straddle groups; 252 threads, R 28
    (16, 16, 192, 0, 1e-5, 2, (48, 252, 13, 14, 1)),     # the narrower slab (Cc 96 would need 26 rows)
    (16, 16, 768, 0, 1e-5, 2, (48, 252, 13, 14, 1)),     # 16 slabs
    # ---- multi-pass
    (16, 16, 520, 2, 1e-5, 2, (0, 130, 64, 0, 4)),       # no slab fits (cpg 260) at HW 256; R 1, 130 threads
    (17, 17, 32, 8, 1e-5, 2, (0, 256, 73, 0, 4)),        # last split 70 of 73, R 32
    (17, 17, 192, 0, 1e-5, 2, (0, 240, 73, 0, 4)),       # R 5, 240 threads
    (15, 21, 64, 0, 1e-5, 2, (0, 256, 79, 0, 4)),        # HW 315 = 5 x 63: a split rule that divides by 63 would say S 5; last split 78 of 79
    (20, 13, 768, 0, 1e-5, 2, (0, 192, 65, 0, 4)),       # R 1, 192 threads
    (33, 32, 128, 32, 1e-6, 2, (0, 256, 66, 0, 16)),     # S 16: the 64-row rule's last step
    (33, 33, 32, 8, 1e-5, 2, (0, 256, 273, 0, 4)),       # the 256-row rule, last split 270 of 273
    (32, 34, 192, 0, 1e-5, 2, (0, 240, 272, 0, 4)),      # 272 rows per split, even
    (33, 33, 1280, 0, 1e-5, 2, (0, 320, 273, 0, 4)),     # R 1, 320 threads
    (66, 66, 32, 8, 1e-5, 1, (0, 256, 257, 0, 17)),      # S 17, last split 244 of 257
]
KINDS = ("plain", "offset", "zero")


def row_id(row):
    H, W, C, G, eps, B, _ = row
    return f"{H}x{W}-C{C}-G{G}" + ("-eps1e-6" if eps != 1e-5 else "")


def groups_of(row):
    return row[3] if row[3] else min(32, row[2] // 4)


@functools.lru_cache(maxsize=8)
def make_case(row, kind):
    """CPU fp32 tensors of a row (NHWC): x (plain: std 2, mean 0.3; offset: the same + 30, so |mean| / std = 15; zero: the first group of image 0 all
    zeros), gamma, beta, ss [B, 2C], dy, addend.  Fixed generator: the same values everywhere.  Shared: do not modify."""
    H, W, C, _, _, B, _ = row
    gen = torch.Generator().manual_seed(zlib.crc32(row_id(row).encode()))
    rn = lambda *s: torch.randn(*s, generator=gen)
    ru = lambda *s: torch.rand(*s, generator=gen) * 2 - 1
    x = rn(B, H, W, C) * 2.0 + 0.3
    n = H * W * (C // groups_of(row))                    # values per group
    if n < 16:
        # the 1x1 row: the deviation of 4 normal values can be tiny (0.2 in this draw), which makes the group ill-conditioned for ANY
        # fp32 arithmetic; an evenly spaced pattern of deviation 1.5 ... 2.5 per group instead
        assert H * W == 1
        pat = torch.linspace(-1.0, 1.0, n)
        pat = pat / pat.square().mean().sqrt()
        x = (pat * (1.5 + ru(B, groups_of(row), 1).abs())).reshape(B, 1, 1, C) + 0.3
    case = dict(gamma=1.0 + 0.2 * ru(C), beta=0.1 * ru(C), ss=0.5 * ru(B, 2 * C), dy=rn(B, H, W, C), addend=rn(B, H, W, C))
    if kind == "offset":
        # (+ 3 on the 1x1 row: with 4 values per group the fp32 torch composition itself is at 5e-6 ... 5e-5 at + 30)
        x = x + (30.0 if n >= 16 else 3.0)
    elif kind == "zero":
        x[0, :, :, :C // groups_of(row)] = 0.0
    else:
        assert kind == "plain"
    case["x"] = x
    return case


def torch_composition(x, gamma, beta, ss, *, groups, eps, silu, keep=None, addend=None, dy=None):
    """The unfused fp32 composition (F.group_norm, addcmul, F.silu, mask) on NHWC tensors, with autograd's gradients: the dict of
    fp64ref.group_norm without the mags."""
    need = dy is not None
    x, gamma, beta = (t.detach().clone().requires_grad_(need) for t in (x, gamma, beta))
    C = x.shape[-1]
    # (contiguous NCHW: torch's channels-last CPU kernel takes E[x^2] - mean^2 in fp32, which loses log2(mean^2 / var) bits)
    z = F.group_norm(x.permute(0, 3, 1, 2).contiguous(), groups, gamma, beta, eps).permute(0, 2, 3, 1)
    wrt = [x, gamma, beta]
    if ss is not None:
        ss = ss.detach().clone().requires_grad_(need)
        z = torch.addcmul(ss[:, C:].reshape(-1, 1, 1, C), z, ss[:, :C].reshape(-1, 1, 1, C) + 1)
        wrt.append(ss)
    y = F.silu(z) if silu else z
    if keep is not None:
        y = y * keep
    out = {"y": y.detach()}
    if need:
        g = torch.autograd.grad(y, wrt, dy)
        out.update(dx=g[0] if addend is None else g[0] + addend, dgamma=g[1], dbeta=g[2])
        if ss is not None:
            out["dss"] = g[3]
    return out
