"""GPU tests of the row reuse of the 3x3 Winograd kernel's producer (conv_wino2d_x6.hip, adm_wino2d_x6_row_reuse) through the C ABI.

With the switch on, a whole K block fetches each of the four patch rows of a tile and chunk once and keeps it in registers across the
four ey passes; with it off every pass fetches its two rows.  Both settings run the same arithmetic on the same values in the same
order, so every case asserts
  1. the whole output buffer (padding included) is BIT-IDENTICAL between the two settings -- a wrong row, sign, chunk or register set
     cannot hide in a tolerance -- and
  2. the output meets the bound of tests/test_hip_conv_epilogue.py (tests/parity.py::close) against an fp64 convolution.
The shapes are about borders and block boundaries, not size: one-tile maps whose halo is all padding, a ragged second pixel tile,
and Cin = 32 / 64 / 96 / 192, which between them give whole blocks, a whole block followed by a partial one, and a lone partial
block under both block lengths (4 chunks for the 64-cout forms, 3 for the 96- and 128-cout forms).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import fill

from test_hip_conv_epilogue import _check, _padded  # noqa: E402  (sentinel-filled buffers; values at parity.close + untouched padding)

pytestmark = pytest.mark.gpu

ALL = (0, 3, 1, "x6")       # adm_wino2d_h3_wide values of the fp16 format (64, 96, 128 couts per workgroup), "x6" = the bf16 format
NARROW = (0, "x6")          # N <= 64, or split-K: the wide forms do not apply
# name: (B, H = W of the output grid, Cin, N, up, workspace floats, forms)
CASES = {
    "h2-c32-n40": (1, 2, 32, 40, 0, 0, NARROW),          # one tile, every halo row and column out of range; one partial block
    "h2-c96-n104": (2, 2, 96, 104, 0, 0, ALL),           # whole blocks of 3 / a whole block of 4 plus a partial one
    "h4-c64-n104": (2, 4, 64, 104, 0, 0, ALL),           # one whole block of 4 / a whole block of 3 plus a partial one
    "h4-c192-n40": (1, 4, 192, 40, 0, 0, NARROW),        # several whole blocks
    "h6-c96-n40": (1, 6, 96, 40, 0, 0, NARROW),          # 9 tiles, interior tile with all four rows valid
    "h6-c192-n192": (5, 6, 192, 192, 0, 0, ALL),         # 45 tiles; whole blocks of both lengths, several of them
    "h8-c192-n104": (5, 8, 192, 104, 0, 0, ALL),         # 80 tiles: a ragged second pixel tile
    "h8-c64-n192": (5, 8, 64, 192, 0, 0, ALL),
    "h8-c32-n192": (2, 8, 32, 192, 0, 0, ALL),           # a lone partial block in every form
    "splitk": (2, 4, 192, 104, 0, 6 * 2 * 16 * 104, NARROW),      # split-K: every split starts its own block sequence
    "up": (2, 8, 96, 104, 1, 0, ALL),                    # fused nearest x2: three passes, keeps its two row loads per stage
}
PARAMS = [(name, form) for name, c in CASES.items() for form in c[6]]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip, ops as _ops
    hip.lib()        # raises if the HIP library is missing: no fallback
    return _ops


@functools.lru_cache(maxsize=None)
def _data(name):
    B, H, cin, N, up, _, _ = CASES[name]
    Hs = H // 2 if up else H
    x = fill.hash_tensor((B, cin, Hs, Hs), f"reuse.x.{name}", 1.0)
    w = fill.hash_tensor((N, cin, 3, 3), f"reuse.w.{name}", 1.0 / (cin * 9) ** 0.5)
    b = fill.hash_tensor((N,), f"reuse.b.{name}", 0.5)
    r = fill.hash_tensor((B, N, H, H), f"reuse.r.{name}", 1.0)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    y64 = F.conv2d(xin.double(), w.double(), None, padding=1)          # fp64 reference, once per shape
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()
    return x, w, b, rows(r), rows(y64)


@functools.lru_cache(maxsize=None)
def _weights(name):
    """(fp16 image, bf16 image, padded cout) of the case's weight, on the GPU"""
    from adm_amd import hip, ops as _ops
    _, _, cin, N, *_ = CASES[name]
    w = _data(name)[1].cuda().contiguous()
    cop, cip = _ops.ceil32(N), _ops.ceil32(cin)
    w2f = torch.empty((16, cop, cip), device="cuda", dtype=torch.float32)
    w2b = torch.empty((16, cip, cop), device="cuda", dtype=torch.float32)
    hip.call("adm_pack_weight_wino2d", hip.ptr(w), hip.ptr(w2f), hip.ptr(w2b), N, cin, cop, cip)
    wh = torch.empty((16, 2, cop, cip), device="cuda", dtype=torch.float16)
    flag = torch.zeros(1, device="cuda", dtype=torch.int32)
    hip.call("adm_split2_f16", hip.ptr(w2f), hip.ptr(wh), cop, cip, _ops.H3_WSCALE, hip.ptr(flag))
    assert int(flag.item()) == 0
    w6 = torch.empty((16, 3, cop, cip), device="cuda", dtype=torch.bfloat16)
    hip.call("adm_split3_bf16", hip.ptr(w2f), hip.ptr(w6), cop, cip)
    return wh, w6, cop


def _launch(ops, name, form, reuse, xd, bd, rd):
    """one launch with the switch at `reuse`; the output buffer [M + tail][N], sentinel-filled before the launch"""
    from adm_amd import hip
    B, H, cin, N, up, ws_n, _ = CASES[name]
    wh, w6, cop = _weights(name)
    yd = _padded(B * H * H, N, N)
    ws = torch.zeros(ws_n, device="cuda", dtype=torch.float32) if ws_n else None
    lib = hip.lib()
    old_reuse = lib.adm_wino2d_x6_row_reuse(reuse)
    old_wide = lib.adm_wino2d_h3_wide(-1)
    try:
        if form == "x6":
            hip.call("adm_conv_fwd_wino2d_x6_up" if up else "adm_conv_fwd_wino2d_x6", hip.ptr(xd), hip.ptr(w6), hip.ptr(bd), hip.ptr(rd),
                     hip.ptr(yd), hip.ptr(ws), ws_n, B, H, H, cin, cin, N, cop, N, N)
        else:
            lib.adm_wino2d_h3_wide(form)
            hip.call("adm_conv_fwd_wino2d_h3", hip.ptr(xd), hip.ptr(wh), hip.ptr(bd), hip.ptr(rd), hip.ptr(yd), hip.ptr(ws), ws_n,
                     B, H, H, cin, cin, N, cop, N, N, hip.ptr(ops.amax_vector(xd)), ops.H3_WSCALE, up)
        torch.cuda.synchronize()
    finally:
        lib.adm_wino2d_h3_wide(old_wide)
        lib.adm_wino2d_x6_row_reuse(old_reuse)
    return yd


@pytest.mark.parametrize("with_bias_res", [False, True], ids=["plain", "bias-res"])
@pytest.mark.parametrize("name,form", PARAMS, ids=[f"{n}-{f}" for n, f in PARAMS])
def test_row_reuse_is_bit_identical_and_within_bound(ops, name, form, with_bias_res):
    from adm_amd import hip
    B, H, cin, N, up, ws_n, _ = CASES[name]
    if ws_n:
        assert hip.lib().adm_wino2d_x6_splitk(B, H, H, cin, N) > 1, "the case is meant to take the split-K path"
    x, _, b, r, y64 = _data(name)
    M = B * H * H
    xd = x.permute(0, 2, 3, 1).contiguous().cuda()                      # [B][Hs][Hs][ldx = Cin]
    bd = b.cuda() if with_bias_res else None
    rd = _padded(M, N, N, r, fill_value=3.0e30) if with_bias_res else None
    y_off = _launch(ops, name, form, 0, xd, bd, rd)
    y_on = _launch(ops, name, form, 1, xd, bd, rd)
    assert hip.lib().adm_wino2d_x6_row_reuse(-1) == 1, "the default (on) is restored"
    diff = y_on.view(torch.int32) != y_off.view(torch.int32)
    assert not bool(diff.any()), f"{int(diff.sum())} of {diff.numel()} elements differ between reuse on and off, first at {diff.nonzero()[0].tolist()}"
    want = y64 + (b.double() + r.double() if with_bias_res else 0.0)
    _check(y_on, want, M, N)
