"""Geometries, data and layouts of the bf16-mode sweep, shared by tests/test_bf16_plan_host.py (CPU) and
tests/test_hip_bf16_accuracy.py (GPU).  A plain helper like gn_cases.py, not a conftest.

The direct bf16 kernels (conv_igemm_bf16.hip, conv_wgrad_bf16.hip) round their operands to bf16 and multiply on
v_mfma_f32_32x32x16_bf16 with fp32 accumulation: products of bf16 values are exact in fp32, so against fp64 of the ROUNDED operands
they are held to the f32 kernel's bars.  Everything here is CPU fp32 and deterministic (oracle.fill.hash_tensor); do not modify what
data() returns -- it is cached and shared.
"""
import functools

import torch

from oracle import fill

import fp64ref

TILES = {0: (128, 128), 1: (128, 96), 2: (64, 64)}          # the forms of adm_conv_fwd_bf16: id -> (BM, BN)

# (B, H, W, Cin, N, ks, up); H x W is the OUTPUT map (the input is H/2 x W/2 when up)
FWD = [
    (3, 5, 7, 64, 96, 3, 0),            # M = 105 ragged for every form; N exact only for the 96-wide form
    (2, 12, 12, 192, 160, 3, 0),        # M = 2 * 128 + 32; N ragged for all three forms; three K chunks per tap
    (1, 16, 16, 64, 128, 1, 0),         # the `full` epilogue of the 128x128 and 64x64 forms
    (1, 16, 24, 128, 192, 3, 0),        # M = 3 * 128, N = 2 * 96: the `full` epilogue of the 128x96 form
    (2, 6, 10, 64, 64, 3, 1),           # fused nearest-x2 from a 3x5 map, both pixel parities
    (1, 1, 2, 64, 64, 3, 0),            # images smaller than the filter
    (2, 1, 1, 128, 64, 3, 0),
]


def epilogues(g, tile):
    """(tiles on the unguarded `full` epilogue, tiles on the guarded one) of a forward geometry on a form: a tile is full when
    m0 + BM <= M and n0 + BN <= N."""
    BM, BN = TILES[tile]
    M, N = g[0] * g[1] * g[2], g[4]
    tiles = -(-M // BM) * -(-N // BN)
    full = (M // BM) * (N // BN)
    return full, tiles - full


# (B, H, W, Cin, Cout, ks, up)
WGRAD = [
    (3, 8, 8, 64, 64, 3, 0),            # FAST, 64x64, three exact stages
    (2, 16, 4, 128, 128, 3, 0),         # FAST with H != W, 128x128
    (3, 4, 8, 160, 96, 3, 0),           # FAST; last Cin tile and second Cout tile half empty; one ragged stage
    (2, 5, 7, 64, 128, 3, 0),           # general path, P = 70
    (1, 64, 2, 128, 64, 3, 0),          # FAST
    (1, 2, 64, 128, 64, 3, 0),          # W > 32: general
    (2, 6, 10, 64, 64, 3, 1),           # up-sampled: general
    (3, 12, 12, 128, 64, 1, 0),         # 1x1, general
    (4, 8, 8, 64, 128, 1, 0),           # 1x1, FAST
    (1, 1, 2, 64, 64, 3, 0),            # images smaller than the filter
    (2, 1, 1, 128, 64, 3, 0),
]
WGRAD_SPLIT = (WGRAD[0], WGRAD[2], WGRAD[3])        # also at explicit splits 2 and 3: the last chunk is then short
WGRAD_AUTO = (5, 16, 16, 64, 64, 3, 0)              # splits 0 (memset) and -1 (pre-zeroed): both atomic two-way splits

# adm_conv_wgrad_bf16_plan(P, Cin, Cout, ks, splits) -> (TM, TN, splits, chunk), and the load path (FAST: power-of-two H and W,
# W <= 32, no up-sampling).  Written from the launcher's rule: TM / TN = 128 where Cout / Cin is a multiple of 128, else 64; chunk =
# ceil(ceil(P / splits) / 64) * 64; splits = ceil(P / chunk).  Auto: min(512 // tiles, ceil(P / 1024)) with tiles = tilesM tilesN ks^2.
WGRAD_PLANS = {
    (WGRAD[0], 1): (64, 64, 1, 192, True),
    (WGRAD[0], 2): (64, 64, 2, 128, True),           # 128 + 64
    (WGRAD[0], 3): (64, 64, 3, 64, True),
    (WGRAD[1], 1): (128, 128, 1, 128, True),
    (WGRAD[2], 1): (64, 64, 1, 128, True),           # P = 96: 64 + 32
    (WGRAD[2], 2): (64, 64, 2, 64, True),            # 64 + 32
    (WGRAD[2], 3): (64, 64, 2, 64, True),            # three asked, chunk 64 -> two
    (WGRAD[3], 1): (128, 64, 1, 128, False),         # P = 70
    (WGRAD[3], 2): (128, 64, 2, 64, False),          # 64 + 6
    (WGRAD[3], 3): (128, 64, 2, 64, False),
    (WGRAD[4], 1): (64, 128, 1, 128, True),
    (WGRAD[5], 1): (64, 128, 1, 128, False),
    (WGRAD[6], 1): (64, 64, 1, 128, False),          # P = 120
    (WGRAD[7], 1): (64, 128, 1, 448, False),         # P = 432
    (WGRAD[8], 1): (128, 64, 1, 256, True),
    (WGRAD[9], 1): (64, 64, 1, 64, True),            # 1 x 2: H and W are powers of two -> FAST
    (WGRAD[10], 1): (64, 128, 1, 64, True),
    (WGRAD_AUTO, 0): (64, 64, 2, 640, True),         # P = 1280: 9 tiles -> 56 splits allowed, ceil(1280 / 1024) = 2 taken
    (WGRAD_AUTO, -1): (64, 64, 2, 640, True),
}


def geom_id(g):
    B, H, W, ci, co, ks, up = g
    return f"B{B}-{H}x{W}-{ci}to{co}-k{ks}{'-up' if up else ''}"


def is_fast(g):
    _, H, W, _, _, _, up = g
    pow2 = lambda v: v & (v - 1) == 0
    return pow2(H) and pow2(W) and W <= 32 and not up


def r16(t):
    """Round to nearest even to bf16 and widen: the values the kernels multiply."""
    return t.to(torch.bfloat16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def data(g):
    """CPU fp32 operands of a geometry, NOT yet rounded: x [B, Hin, Win, Cin] in [-1, 1), w [N, Cin, ks, ks] in +-K^-1/2, bias [N] in
    +-0.1, res and dy [B, H, W, N] in [-1, 1).  Zero-mean hashed values: the sums cancel like a trained layer's, and an fp32
    accumulation in any order stays far inside bar A (test_bf16_plan_host.py checks that)."""
    B, H, W, ci, co, ks, up = g
    Hin, Win = (H // 2, W // 2) if up else (H, W)
    tag = geom_id(g)
    return dict(x=fill.hash_tensor((B, Hin, Win, ci), "bf16acc.x." + tag, 1.0),
                w=fill.hash_tensor((co, ci, ks, ks), "bf16acc.w." + tag, (ci * ks * ks) ** -0.5),
                bias=fill.hash_tensor((co,), "bf16acc.b." + tag, 0.1),
                res=fill.hash_tensor((B, H, W, co), "bf16acc.r." + tag, 1.0),
                dy=fill.hash_tensor((B, H, W, co), "bf16acc.g." + tag, 1.0))


@functools.lru_cache(maxsize=None)
def references(g):
    """fp64 (ref, mag) of the three outputs of a geometry, each on the operands rounded as its kernel rounds them: y from (x, w) with
    the fp32 bias and residual; dx from (dy, w); dw from (dy, x).  NHWC / OIHW, CPU; computed once per geometry and shared."""
    d = data(g)
    up = bool(g[6])
    return dict(y=fp64ref.conv(r16(d["x"]), r16(d["w"]), d["bias"], d["res"], up=up)["y"],
                y0=fp64ref.conv(r16(d["x"]), r16(d["w"]), up=up)["y"],
                dx=fp64ref.conv(d["x"], r16(d["w"]), dy=r16(d["dy"]), up=up)["dx"],
                dw=fp64ref.conv(r16(d["x"]), d["w"], dy=r16(d["dy"]), up=up)["dw"])


def fwd_operand(w):
    """The forward B operand as the kernels read it, from OIHW: row n, column tap * Cin + c (tap = ky * ks + kx)."""
    co, ci, ks, _ = w.shape
    return w.permute(0, 2, 3, 1).reshape(co, ks * ks * ci).contiguous()


def bwd_operand(w):
    """The data-gradient operand: the same conv over dy with cin and cout exchanged and the taps flipped: row c, column tap * Cout + n
    holds w[n][c][ks - 1 - ky][ks - 1 - kx]."""
    co, ci, ks, _ = w.shape
    return w.flip(2, 3).permute(1, 2, 3, 0).reshape(ci, ks * ks * co).contiguous()


def production_shapes():
    """(M, N) of every conv the CIFAR UNet of BASELINE configs[2] can send to adm_conv_fwd_bf16 at the per-GPU batch 128: M = 128 H^2
    for H in {32, 16, 8, 4}; N over the padded widths of the model's conv weights in both directions -- the forward writes ceil32(cout)
    columns and runs in the mode where ceil32(cin) % 64 == 0, the data gradient writes ceil32(cin) where ceil32(cout) % 64 == 0."""
    from oracle import unet_ref
    c32 = lambda n: -(-n // 32) * 32
    widths = set()
    for name, s in unet_ref.param_shapes(unet_ref.default_cfg()).items():
        if name.endswith(".weight") and len(s) == 4:
            cop, cip = c32(s[0]), c32(s[1])
            if cip % 64 == 0:
                widths.add(cop)
            if cop % 64 == 0:
                widths.add(cip)
    return [(128 * H * H, N) for H in (32, 16, 8, 4) for N in sorted(widths)]
