"""GPU tests of the output epilogues of the split-format conv kernels (conv_wino2d_x6.hip, conv_gemm_x6.hip) through the C ABI.

The Python path always passes ldy = ldr = N = a multiple of 32; here the raw entry points get the strides and ragged edges it never
produces.  Every case checks, against an fp64 reference computed on the CPU,
  * the values of the valid region at the tolerance of tests/parity.py::close, and
  * every byte outside it: the output buffer is pre-filled with a sentinel, and the padding columns n in [N, ldy) and the rows past
    the end must still hold it.
The epilogue has one body with a residual (one batch of loads, then one batch of stores) and one without (stores only);
test_*_bodies_agree pins the arithmetic order across the two.

A bound vector's value is the maximum of its slots (include/adm_hip.h: every wave raises a slot of its own), so the 1x1 cases
compare max(amax_y) -- not slot 0 alone -- with max |y| of the valid region, exactly."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

from oracle import fill

from parity import close  # noqa: E402  (tests/parity.py: the north_star tolerance, elementwise)

pytestmark = pytest.mark.gpu

SENTINEL = -7.015625e8      # (exact in f32)
TAIL_ROWS = 3               # rows of ldy floats allocated past the end of y


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip, ops as _ops
    hip.lib()        # raises if the HIP library is missing: no fallback
    return _ops


def _padded(rows_valid, n, ld, src=None, fill_value=SENTINEL, tail=TAIL_ROWS):
    """[rows_valid + tail][ld] f32 on the GPU, filled with fill_value; src ([rows_valid][n]) in the valid region"""
    buf = torch.full((rows_valid + tail, ld), fill_value, dtype=torch.float32)
    if src is not None:
        buf[:rows_valid, :n] = src
    return buf.cuda()


def _check(y_buf, want, rows_valid, n):
    """values of the valid region against fp64, and the sentinel everywhere else, bit for bit"""
    got = y_buf.cpu()
    close(got[:rows_valid, :n], want)
    outside = got.clone()
    outside[:rows_valid, :n] = SENTINEL
    bad = outside.view(torch.int32) != torch.full_like(outside, SENTINEL).view(torch.int32)
    assert not bool(bad.any()), f"{int(bad.sum())} elements outside the valid region were written, first at {bad.nonzero()[0].tolist()}"
    return got[:rows_valid, :n].clone()


# ------------------------------------------------------------------------------------------------------------------ 3x3
# (name, B, H = W of the OUTPUT grid, Cin, N, ldy, ldr, up, workspace floats, forms): forms = values of adm_wino2d_h3_wide (0: 64
# couts per workgroup, 3: 96, 1: 128; the wide forms need N > 64 and no split-K) for the fp16 format, "x6" = the bf16 format
CASES3 = {
    "ragged9": (1, 6, 32, 40, 48, 56, 0, 0, (0, "x6")),              # 9 tiles of 64 per workgroup, ragged couts
    "tile2": (5, 8, 32, 100, 104, 112, 0, 0, (0, 3, 1, "x6")),       # 80 tiles: a ragged second pixel tile; 96 form: 4 couts in tile 2
    "up": (2, 8, 32, 72, 80, 84, 1, 0, (0, 3, 1, "x6")),             # the fused nearest x2 (source 4 x 4)
    "splitk": (2, 4, 128, 64, 68, 72, 0, 8192, (0, "x6")),           # split-K: partials through the no-residual body, then the reduce
}


@functools.lru_cache(maxsize=None)
def _data3(name):
    B, H, cin, N, ldy, ldr, up, ws_n, _ = CASES3[name]
    Hs = H // 2 if up else H
    x = fill.hash_tensor((B, cin, Hs, Hs), f"epi3.x.{name}", 1.0)
    w = fill.hash_tensor((N, cin, 3, 3), f"epi3.w.{name}", 1.0 / (cin * 9) ** 0.5)
    b = fill.hash_tensor((N,), f"epi3.b.{name}", 0.5)
    r = fill.hash_tensor((B, N, H, H), f"epi3.r.{name}", 1.0)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    y64 = F.conv2d(xin.double(), w.double(), None, padding=1)          # fp64 reference, once per shape
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()
    return x, w, b, rows(r), rows(y64), b.double()


@functools.lru_cache(maxsize=None)
def _weights3(name):
    """(f32 Winograd planes [16][cop][cip], fp16 image, bf16 image, cop) of the case's weight, on the GPU"""
    from adm_amd import hip, ops as _ops
    _, _, cin, N, *_ = CASES3[name]
    w = _data3(name)[1].cuda().contiguous()
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


def _run3(ops, name, form, with_bias, with_res):
    from adm_amd import hip
    B, H, cin, N, ldy, ldr, up, ws_n, _ = CASES3[name]
    x, _, b, r, y64, b64 = _data3(name)
    wh, w6, cop = _weights3(name)
    M = B * H * H
    xd = x.permute(0, 2, 3, 1).contiguous().cuda()                      # [B][Hs][Hs][ldx = Cin]
    bd = b.cuda() if with_bias else None
    rd = _padded(M, N, ldr, r, fill_value=3.0e30) if with_res else None     # (padding of the residual: never to be read into y)
    yd = _padded(M, N, ldy)
    ws = torch.zeros(ws_n, device="cuda", dtype=torch.float32) if ws_n else None
    if form == "x6":
        hip.call("adm_conv_fwd_wino2d_x6_up" if up else "adm_conv_fwd_wino2d_x6", hip.ptr(xd), hip.ptr(w6), hip.ptr(bd), hip.ptr(rd),
                 hip.ptr(yd), hip.ptr(ws), ws_n, B, H, H, cin, cin, N, cop, ldy, ldr)
    else:
        old = hip.lib().adm_wino2d_h3_wide(form)
        try:
            hip.call("adm_conv_fwd_wino2d_h3", hip.ptr(xd), hip.ptr(wh), hip.ptr(bd), hip.ptr(rd), hip.ptr(yd), hip.ptr(ws), ws_n,
                     B, H, H, cin, cin, N, cop, ldy, ldr, hip.ptr(ops.amax_vector(xd)), ops.H3_WSCALE, up)
        finally:
            hip.lib().adm_wino2d_h3_wide(old)
    torch.cuda.synchronize()
    want = y64 + (b64 if with_bias else 0.0) + (r.double() if with_res else 0.0)
    return _check(yd, want, M, N), r


PARAMS3 = [(name, form) for name, c in CASES3.items() for form in c[8]]


@pytest.mark.parametrize("with_bias,with_res", list(itertools.product((False, True), repeat=2)))
@pytest.mark.parametrize("name,form", PARAMS3, ids=[f"{n}-{f}" for n, f in PARAMS3])
def test_conv3x3_epilogue_strides_and_edges(ops, name, form, with_bias, with_res):
    if CASES3[name][7]:
        B, H, cin, N = CASES3[name][:4]
        from adm_amd import hip
        assert hip.lib().adm_wino2d_x6_splitk(B, H, H, cin, N) > 1, "the case is meant to take the split-K path"
    _run3(ops, name, form, with_bias, with_res)


@pytest.mark.parametrize("form", [0, 3, "x6"])
def test_conv3x3_epilogue_bodies_agree(ops, form):
    """with residual r == (without residual) + r, element for element in f32: the two epilogue bodies keep one arithmetic order"""
    y0, r = _run3(ops, "tile2", form, True, False)
    y1, _ = _run3(ops, "tile2", form, True, True)
    assert torch.equal(y1, y0 + r)


# ------------------------------------------------------------------------------------------------------------------ 1x1
G_M, G_N, G_WROWS, G_LDY, G_LDR = 130, 132, 256, 136, 140      # second pixel tile: 2 rows; second cout tile: 4 valid columns


@functools.lru_cache(maxsize=None)
def _data1(K):
    x = fill.hash_tensor((G_M, K), f"epi1.x.{K}", 1.0)
    w = fill.hash_tensor((G_WROWS, K), f"epi1.w.{K}", 1.0 / K ** 0.5)      # rows N .. wrows - 1: computed by the kernel, never stored
    b = fill.hash_tensor((G_N,), f"epi1.b.{K}", 0.5)
    r = fill.hash_tensor((G_M, G_N), f"epi1.r.{K}", 1.0)
    y64 = x.double() @ w[:G_N].double().t() + b.double()
    return x, w, b, r, y64


def _run1(ops, K, fmt, with_res):
    from adm_amd import hip
    x, w, b, r, y64 = _data1(K)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    rd = _padded(G_M, G_N, G_LDR, r, fill_value=3.0e30) if with_res else None
    yd = _padded(G_M, G_N, G_LDY)
    amax_y = torch.zeros(ops.AMAX_FLOATS, device="cuda", dtype=torch.float32)
    if fmt == "h3":
        img = torch.empty((K // 16, 2, G_WROWS, 16), device="cuda", dtype=torch.float16)
        flag = torch.zeros(1, device="cuda", dtype=torch.int32)
        hip.call("adm_split2_rows_f16", hip.ptr(wd), hip.ptr(img), G_WROWS, K, K, ops.H3_WSCALE, hip.ptr(flag))
        assert int(flag.item()) == 0
        hip.call("adm_gemm_x6_h3", hip.ptr(xd), hip.ptr(img), hip.ptr(bd), hip.ptr(rd), hip.ptr(yd), G_M, K, K, G_N, G_WROWS, G_LDY, G_LDR,
                 hip.ptr(ops.amax_vector(xd)), ops.H3_WSCALE, hip.ptr(amax_y))
    else:
        img = torch.empty((K // 16, 3, G_WROWS, 16), device="cuda", dtype=torch.bfloat16)
        hip.call("adm_split3_rows", hip.ptr(wd), hip.ptr(img), G_WROWS, K, K)
        hip.call("adm_gemm_x6_amax", hip.ptr(xd), hip.ptr(img), hip.ptr(bd), hip.ptr(rd), hip.ptr(yd), G_M, K, K, G_N, G_WROWS, G_LDY, G_LDR,
                 hip.ptr(amax_y))
    torch.cuda.synchronize()
    got = _check(yd, y64 + (r.double() if with_res else 0.0), G_M, G_N)
    assert float(amax_y.max()) == float(got.abs().max()), "the bound vector is max |y| over the valid region, exactly"
    return got, r


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("K", [32, 96])      # 32: a single stage (only the last-stage wait path runs)
@pytest.mark.parametrize("fmt", ["h3", "x6"])
def test_conv1x1_epilogue_strides_and_edges(ops, fmt, K, with_res):
    _run1(ops, K, fmt, with_res)


@pytest.mark.parametrize("fmt", ["h3", "x6"])
def test_conv1x1_epilogue_bodies_agree(ops, fmt):
    y0, r = _run1(ops, 96, fmt, False)
    y1, _ = _run1(ops, 96, fmt, True)
    assert torch.equal(y1, y0 + r)
