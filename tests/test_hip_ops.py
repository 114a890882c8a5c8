"""GPU parity tests, op level: every HIP kernel (through the C ABI) against plain PyTorch fp32 on CPU.

Tolerance: north_star's rtol 1e-3 / atol 1e-4 (fp32), scaled by the tensor's magnitude where a
gradient's natural scale is far from 1."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import fill, unet_ref

from parity import close  # noqa: E402  (tests/parity.py: the north_star tolerance, elementwise)

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-3, 1e-4


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip, ops as _ops
    hip.lib()        # raises if the HIP library is missing: no fallback
    return _ops


def dev(t):
    return t.cuda().contiguous()


def nhwc(t):
    return dev(t.permute(0, 2, 3, 1))


def nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2)


def pad_c(t, c):
    out = torch.zeros(t.shape[0], c, *t.shape[2:])
    out[:, : t.shape[1]] = t
    return out


@pytest.mark.parametrize("cin,cout,H,ks,up,tile", [
    (32, 64, 8, 3, False, -1), (64, 96, 16, 3, False, 1), (64, 128, 16, 3, False, 0), (96, 64, 8, 1, False, 2),
    (64, 32, 8, 3, False, 3), (64, 64, 4, 3, True, -1), (192, 192, 32, 3, False, -1), (3, 64, 16, 3, False, -1),
    (64, 3, 16, 3, False, -1), (384, 1, 4, 1, False, -1),
    (32, 64, 12, 3, False, -1), (32, 32, 64, 3, False, -1), (64, 32, 6, 3, True, -1),   # non-power-of-two / W > 32: generic paths
    (384, 384, 4, 3, False, -1), (768, 384, 4, 3, False, -1), (384, 96, 4, 1, False, -1)])   # small M: deterministic split-K
def test_conv_forward_backward(ops, cin, cout, H, ks, up, tile):
    B = 3
    x = fill.hash_tensor((B, cin, H, H), f"cx{cin}{cout}", 1.0)
    w = fill.hash_tensor((cout, cin, ks, ks), f"cw{cin}{cout}", 1.0 / math.sqrt(cin * ks * ks))
    b = fill.hash_tensor((cout,), f"cb{cin}{cout}", 0.5)
    Ho = 2 * H if up else H
    r = fill.hash_tensor((B, cout, Ho, Ho), f"cr{cin}{cout}", 1.0)
    gy = fill.hash_tensor((B, cout, Ho, Ho), f"cg{cin}{cout}", 1.0)
    xr, wr, br, rr = [t.clone().requires_grad_(True) for t in (x, w, b, r)]
    xin = F.interpolate(xr, scale_factor=2, mode="nearest") if up else xr
    y_ref = F.conv2d(xin, wr, br, padding=ks // 2) + rr
    (y_ref * gy).sum().backward()

    cip, cop = ops.ceil32(cin), ops.ceil32(cout)
    xd = nhwc(pad_c(x, cip)).requires_grad_(True)
    wd, bd = dev(w).requires_grad_(True), dev(b).requires_grad_(True)
    rd = nhwc(pad_c(r, cop)).requires_grad_(True)
    y = ops.conv2d(xd, wd, bd, rd, up=up, tile=tile)
    assert y.shape == (B, Ho, Ho, cop)
    close(nchw(y)[:, :cout], y_ref)
    if cop > cout:
        assert float(y.detach()[..., cout:].abs().max()) == 0.0
    (y * nhwc(pad_c(gy, cop))).sum().backward()
    close(nchw(xd.grad)[:, :cin], xr.grad)
    close(wd.grad, wr.grad)
    close(bd.grad, br.grad)
    close(nchw(rd.grad)[:, :cout], rr.grad)


@pytest.mark.parametrize("B,cin,cout,H,W,up", [(3, 32, 32, 8, 8, False), (2, 64, 96, 5, 6, False), (1, 3, 64, 16, 16, False),
                                               (2, 96, 3, 4, 32, False), (4, 192, 192, 16, 16, False), (1, 32, 32, 1, 2, False),
                                               (2, 64, 32, 4, 4, True), (3, 32, 96, 8, 4, True), (1, 96, 64, 3, 5, True),
                                               (2, 384, 384, 8, 8, True)])
def test_conv_winograd_forward_backward(ops, monkeypatch, B, cin, cout, H, W, up):
    """The F(2,3) Winograd kernel (normally chosen for M >= 8192) on small shapes: odd heights, channel padding on both
    sides, width 2, bias + residual; forward and the data gradient go through it, the weight gradient is the shared
    kernel.  Also checked against the direct kernel, which must agree to rounding."""
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    monkeypatch.setattr(ops, "WINOGRAD", True)
    monkeypatch.setattr(ops, "WINOGRAD2D", False)       # the 1-D kernel under test (even-height shapes would take the 2-D one)
    x = fill.hash_tensor((B, cin, H, W), f"wx{cin}{cout}", 1.0)
    w = fill.hash_tensor((cout, cin, 3, 3), f"ww{cin}{cout}", 1.0 / math.sqrt(cin * 9))
    b = fill.hash_tensor((cout,), f"wb{cin}{cout}", 0.5)
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)          # up: the reference's fused nearest x2 (Conv2d(up=True))
    r = fill.hash_tensor((B, cout, Ho, Wo), f"wr{cin}{cout}", 1.0)
    gy = fill.hash_tensor((B, cout, Ho, Wo), f"wg{cin}{cout}", 1.0)
    xr, wr, br, rr = [t.clone().requires_grad_(True) for t in (x, w, b, r)]
    xin = F.interpolate(xr, scale_factor=2, mode="nearest") if up else xr
    y_ref = F.conv2d(xin, wr, br, padding=1) + rr
    (y_ref * gy).sum().backward()
    cip, cop = ops.ceil32(cin), ops.ceil32(cout)
    xd = nhwc(pad_c(x, cip)).requires_grad_(True)
    wd, bd = dev(w).requires_grad_(True), dev(b).requires_grad_(True)
    rd = nhwc(pad_c(r, cop)).requires_grad_(True)
    y = ops.conv2d(xd, wd, bd, rd, up=up)
    assert wd._adm_packed.wf is not None, "the Winograd path was not taken"
    close(nchw(y)[:, :cout], y_ref)
    if cop > cout:
        assert float(y.detach()[..., cout:].abs().max()) == 0.0
    (y * nhwc(pad_c(gy, cop))).sum().backward()
    close(nchw(xd.grad)[:, :cin], xr.grad)
    close(wd.grad, wr.grad)
    close(bd.grad, br.grad)
    monkeypatch.setattr(ops, "WINOGRAD", False)
    with torch.no_grad():
        yd = ops.conv2d(xd.detach(), dev(w), dev(b), rd.detach(), up=up)
    assert float((y.detach() - yd).abs().max()) <= 1e-5 * float(yd.abs().max())


@pytest.mark.parametrize("B,cin,cout,H,W", [(3, 32, 32, 8, 8), (2, 64, 96, 6, 10), (1, 3, 64, 16, 16), (2, 96, 3, 4, 32), (4, 192, 192, 16, 16),
                                            (1, 32, 32, 2, 2), (2, 384, 384, 8, 8), (8, 64, 96, 32, 32), (2, 768, 384, 16, 16),
                                            (130, 32, 64, 2, 4)])
@pytest.mark.parametrize("variant", [0, 1])
def test_conv_winograd_2d_forward_backward(ops, monkeypatch, request, B, cin, cout, H, W, variant):
    """The 2-D F(2x2,3x3) kernel (conv_wino2d.hip; 2.25x fewer MFMA flops): forward and data gradient against F.conv2d on the CPU
    and against the direct kernel; channel padding on both sides, 2x2 images, ragged tile counts, bias + residual."""
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    monkeypatch.setattr(ops, "WINOGRAD", True)
    monkeypatch.setattr(ops, "WINOGRAD2D", True)
    monkeypatch.setattr(ops, "BF16X6", False)                 # the f32-MFMA kernels of conv_wino2d.hip (ADM_BF16X6=0)
    from adm_amd import hip as _hip
    old_variant = _hip.lib().adm_wino2d_variant(variant)      # 0: symmetric kernel, 1: wave-specialised kernel
    request.addfinalizer(lambda: _hip.lib().adm_wino2d_variant(old_variant))
    x = fill.hash_tensor((B, cin, H, W), f"w2x{cin}{cout}{H}", 1.0)
    w = fill.hash_tensor((cout, cin, 3, 3), f"w2w{cin}{cout}", 1.0 / math.sqrt(cin * 9))
    b = fill.hash_tensor((cout,), f"w2b{cin}{cout}", 0.5)
    r = fill.hash_tensor((B, cout, H, W), f"w2r{cin}{cout}{H}", 1.0)
    gy = fill.hash_tensor((B, cout, H, W), f"w2g{cin}{cout}{H}", 1.0)
    xr, wr, br, rr = [t.clone().requires_grad_(True) for t in (x, w, b, r)]
    y_ref = F.conv2d(xr, wr, br, padding=1) + rr
    (y_ref * gy).sum().backward()
    cip, cop = ops.ceil32(cin), ops.ceil32(cout)
    xd = nhwc(pad_c(x, cip)).requires_grad_(True)
    wd, bd = dev(w).requires_grad_(True), dev(b).requires_grad_(True)
    rd = nhwc(pad_c(r, cop)).requires_grad_(True)
    monkeypatch.setattr(ops, "PROFILE", [])
    y = ops.conv2d(xd, wd, bd, rd)
    assert wd._adm_packed.w2f is not None and wd._adm_packed.wf is None, "the 2-D Winograd path was not taken"
    close(nchw(y)[:, :cout], y_ref)
    if cop > cout:
        assert float(y.detach()[..., cout:].abs().max()) == 0.0
    (y * nhwc(pad_c(gy, cop))).sum().backward()
    assert [rec[0] for rec in ops.PROFILE].count("wino2") == 2          # forward + data gradient
    close(nchw(xd.grad)[:, :cin], xr.grad)
    close(wd.grad, wr.grad)
    close(bd.grad, br.grad)
    close(nchw(rd.grad)[:, :cout], rr.grad)
    monkeypatch.setattr(ops, "WINOGRAD", False)
    with torch.no_grad():
        yd = ops.conv2d(xd.detach(), dev(w), dev(b), rd.detach())
        assert float((y.detach() - yd).abs().max()) <= 2e-5 * float(yd.abs().max())


@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("B,cin,cout,H,W", [(3, 32, 32, 8, 8), (2, 64, 96, 6, 10), (1, 3, 64, 16, 16), (4, 192, 192, 16, 16), (1, 32, 32, 2, 2),
                                            (2, 384, 384, 8, 8), (8, 64, 96, 32, 32), (130, 32, 64, 2, 4), (2, 96, 64, 3, 5)])
def test_conv_x6_forward_backward(ops, monkeypatch, B, cin, cout, H, W, up):
    """The default 3x3 path (conv_wino2d_x6.hip): the 2-D Winograd convolution with every f32 product carried by six bf16 MFMAs on
    the exact three-term split of both operands -- forward, data gradient and (conv_wgrad_x6.hip, power-of-two sizes) weight gradient,
    plain and with the fused nearest x2 up-sampling of Conv2d(up=True) (H x W is then the INPUT size).  Same parity bar as the
    f32-MFMA kernels, against F.conv2d on the CPU."""
    if not up and (H % 2 or W % 2):
        pytest.skip("odd sizes take the 1-D kernels")
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    monkeypatch.setattr(ops, "WINOGRAD", True)
    monkeypatch.setattr(ops, "WINOGRAD2D", True)
    monkeypatch.setattr(ops, "BF16X6", True)
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    x = fill.hash_tensor((B, cin, H, W), f"x6x{cin}{cout}{H}", 1.0)
    w = fill.hash_tensor((cout, cin, 3, 3), f"x6w{cin}{cout}", 1.0 / math.sqrt(cin * 9))
    b = fill.hash_tensor((cout,), f"x6b{cin}{cout}", 0.5)
    r = fill.hash_tensor((B, cout, Ho, Wo), f"x6r{cin}{cout}{H}", 1.0)
    gy = fill.hash_tensor((B, cout, Ho, Wo), f"x6g{cin}{cout}{H}", 1.0)
    xr, wr, br, rr = [t.clone().requires_grad_(True) for t in (x, w, b, r)]
    xin = F.interpolate(xr, scale_factor=2, mode="nearest") if up else xr
    y_ref = F.conv2d(xin, wr, br, padding=1) + rr
    (y_ref * gy).sum().backward()
    cip, cop = ops.ceil32(cin), ops.ceil32(cout)
    xd = nhwc(pad_c(x, cip)).requires_grad_(True)
    wd, bd = dev(w).requires_grad_(True), dev(b).requires_grad_(True)
    rd = nhwc(pad_c(r, cop)).requires_grad_(True)
    monkeypatch.setattr(ops, "PROFILE", [])
    y = ops.conv2d(xd, wd, bd, rd, up=up)
    assert wd._adm_packed.w2f6 is not None, "the split-bf16 path was not taken"
    close(nchw(y)[:, :cout], y_ref)
    (y * nhwc(pad_c(gy, cop))).sum().backward()
    kinds = [rec[0] for rec in ops.PROFILE]
    assert kinds.count("wino2x6") == 2                                   # forward + data gradient
    pow2 = lambda v: v & (v - 1) == 0
    if pow2(Ho) and pow2(Wo):
        assert kinds.count("wgrad_wino2x6") == 1
    close(nchw(xd.grad)[:, :cin], xr.grad)
    close(wd.grad, wr.grad)
    close(bd.grad, br.grad)
    close(nchw(rd.grad)[:, :cout], rr.grad)


@pytest.mark.parametrize("B,cin,cout,H,qkv,with_res", [(8, 384, 1152, 32, True, False), (8, 384, 384, 32, False, True), (9, 192, 384, 31, False, False),
                                                        (16, 768, 128, 24, False, True), (8, 32, 128, 32, False, False), (8, 128, 96, 32, False, True),
                                                        (8, 576, 192, 32, False, True), (8, 192, 576, 32, False, False)])
def test_conv1x1_x6_forward_backward(ops, monkeypatch, B, cin, cout, H, qkv, with_res):
    """1x1 convs with >= 2048 pixels (GEMM_X6_MIN_M) run on conv_gemm_x6.hip (f32 products as six bf16 MFMAs on the exact three-term split): forward
    (bias, residual, the qkv row permutation), data gradient, and -- through the direct kernels -- weight / bias gradients, against
    F.conv2d on the CPU; ragged pixel counts; then the weights are changed in place and refreshed by repack_all()."""
    monkeypatch.setattr(ops, "BF16X6", True)
    monkeypatch.setattr(ops, "GEMM_WGRAD_X6", True)          # (the default)
    x = fill.hash_tensor((B, cin, H, H), f"g6x{cin}{cout}", 1.0)
    w = fill.hash_tensor((cout, cin, 1, 1), f"g6w{cin}{cout}", 1.0 / math.sqrt(cin))
    b = fill.hash_tensor((cout,), f"g6b{cin}{cout}", 0.5)
    r = fill.hash_tensor((B, cout, H, H), f"g6r{cin}{cout}", 1.0)
    gy = fill.hash_tensor((B, cout, H, H), f"g6g{cin}{cout}", 1.0)
    xr, wr, br = [t.clone().requires_grad_(True) for t in (x, w, b)]
    y_ref = F.conv2d(xr, wr, br) + (r if with_res else 0)
    (y_ref * gy).sum().backward()
    xd = nhwc(x).requires_grad_(True)
    wd, bd = torch.nn.Parameter(dev(w)), torch.nn.Parameter(dev(b))
    monkeypatch.setattr(ops, "PROFILE", [])
    y = ops.conv2d(xd, wd, bd, nhwc(r) if with_res else None, qkv=qkv)
    fwd_x6 = ops.ceil32(cout) >= 128                       # fewer than 128 couts stay on the f32 kernel
    assert [rec[0] for rec in ops.PROFILE].count("gemmx6") == int(fwd_x6) and (wd._adm_packed.g6f is not None) == fwd_x6
    yn = nchw(y)
    if qkv:      # kernel rows are (head, {q,k,v}, c); the reference interleaves (head, c, {q,k,v}) (uncond_unet.py:205)
        heads = cout // 192
        yn = yn.reshape(B, heads, 3, 64, H, H).permute(0, 1, 3, 2, 4, 5).reshape(B, cout, H, H)
    close(yn, y_ref)
    if not qkv:
        monkeypatch.setattr(ops, "PROFILE", [])
        (y * nhwc(gy)).sum().backward()
        assert [rec[0] for rec in ops.PROFILE].count("gemmx6") == (1 if cin >= 128 else 0)       # the data gradient (N = Cin)
        assert [rec[0] for rec in ops.PROFILE].count("wgrad_gemmx6") == 1    # the weight (+ bias) gradient: conv_wgrad_x6.hip MODE 1
        close(nchw(xd.grad), xr.grad)
        close(wd.grad, wr.grad)
        close(bd.grad, br.grad)
    with torch.no_grad():
        wd.data.mul_(0.5).add_(0.02)
    ops.repack_all()
    if not fwd_x6 and cin < 128:
        return
    y2 = ops.conv2d(xd.detach(), wd, bd, nhwc(r) if with_res else None, qkv=qkv)
    if not qkv:
        close(nchw(y2), F.conv2d(x, wd.detach().cpu(), b) + (r if with_res else 0))
    assert not torch.equal(y2, y.detach())


def test_conv_x6_weights_follow_repack_all(ops, monkeypatch):
    """The fused optimiser rewrites parameters through raw pointers and refreshes every packed operand with one launch
    (ops.repack_all): the split-bf16 images must follow, bit for bit as adm_split3_bf16 would produce them."""
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    monkeypatch.setattr(ops, "WINOGRAD", True)
    monkeypatch.setattr(ops, "WINOGRAD2D", True)
    monkeypatch.setattr(ops, "BF16X6", True)
    x = fill.hash_tensor((2, 64, 8, 8), "rpx", 1.0)
    w = torch.nn.Parameter(dev(fill.hash_tensor((96, 64, 3, 3), "rpw", 0.05)))
    y0 = ops.conv2d(nhwc(x), w, None)
    pk = w._adm_packed
    assert pk.w2f6 is not None
    with torch.no_grad():
        w.data.mul_(1.5).add_(0.01)              # in place, as the optimiser kernel does (same storage)
    ops.repack_all()
    assert w._adm_packed is pk
    y1 = ops.conv2d(nhwc(x), w, None)
    close(nchw(y1)[:, :96], F.conv2d(x, w.detach().cpu(), padding=1))
    assert not torch.equal(y0, y1)
    assert pk.w2f is None            # only the splits are kept: the f32 planes would be rewritten by every repack and never read
    want = torch.empty_like(pk.w2f6)
    from adm_amd import hip as _hip
    w2f, w2b = torch.empty((16, 96, 64), device=w.device), torch.empty((16, 64, 96), device=w.device)
    _hip.call("adm_pack_weight_wino2d", w.detach().data_ptr(), w2f.data_ptr(), w2b.data_ptr(), 96, 64, 96, 64)
    _hip.call("adm_split3_bf16", w2f.data_ptr(), want.data_ptr(), w2f.shape[1], w2f.shape[2])
    assert torch.equal(want.view(torch.int16), pk.w2f6.view(torch.int16))


def test_conv_x6_error_vs_fp64(ops, monkeypatch):
    """The six-product bf16 emulation must be as accurate as the f32 MFMA kernel it replaces: both are compared with an fp64
    convolution on zero-mean data AND on all-positive data (no cancellation: the worst case for accumulated rounding)."""
    B, C, H = 4, 384, 16
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    monkeypatch.setattr(ops, "WINOGRAD", True)
    monkeypatch.setattr(ops, "WINOGRAD2D", True)
    for positive in (False, True):
        x = fill.hash_tensor((B, C, H, H), "e64x", 1.0)
        w = fill.hash_tensor((C, C, 3, 3), "e64w", 0.02)
        if positive:
            x, w = x.abs(), w.abs()
        ref = F.conv2d(x.double(), w.double(), padding=1)
        scale = float(F.conv2d(x.double().abs(), w.double().abs(), padding=1).max())
        err = {}
        for mode in (False, True):
            monkeypatch.setattr(ops, "BF16X6", mode)
            wd = dev(w)
            y = ops.conv2d(nhwc(x), wd, None)
            assert (wd._adm_packed.w2f6 is not None) == mode
            err[mode] = float((nchw(y).double().cpu() - ref).abs().max()) / scale
        print(f"positive={positive}: max|err| / max sum|ab|: f32 MFMA {err[False]:.3e}, six bf16 products {err[True]:.3e}")
        assert err[True] <= max(1.5 * err[False], 2e-7), err


@pytest.mark.parametrize("B,cin,cout,H,W,up,force", [
    (8, 64, 96, 32, 32, False, False),      # M = 8192: the Winograd weight-gradient kernel is selected BY DEFAULT
    (8, 96, 64, 16, 16, True, False),       # fused nearest x2 (decoder up-conv): grid 32x32, M = 8192, default selection
    (2, 192, 192, 32, 32, False, True),     # channel counts of the CIFAR network
    (1, 32, 32, 1, 2, False, True),         # the 1x2 image that faulted in round 1 (negative shifted descriptor size)
    (1, 32, 64, 2, 2, False, True), (3, 3, 32, 2, 4, False, True), (2, 32, 32, 1, 1, True, True)])
def test_conv_wgrad_winograd_op_level(ops, monkeypatch, B, cin, cout, H, W, up, force):
    """wgrad_wino_kernel (F(3,2) weight gradient + fused bias gradient) on its own against F.conv2d's autograd on the CPU:
    shapes that select it by default plus tiny-image edge cases.  The launch record proves which kernel ran."""
    if force:
        monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    monkeypatch.setattr(ops, "WINOGRAD", True)
    x = fill.hash_tensor((B, cin, H, W), f"gwx{cin}{cout}{H}", 1.0)
    w = fill.hash_tensor((cout, cin, 3, 3), f"gww{cin}{cout}", 1.0 / math.sqrt(cin * 9))
    b = fill.hash_tensor((cout,), f"gwb{cin}{cout}", 0.5)
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    gy = fill.hash_tensor((B, cout, Ho, Wo), f"gwg{cin}{cout}{H}", 1.0)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    (F.conv2d(xin, wr, br, padding=1) * gy).sum().backward()
    cip, cop = ops.ceil32(cin), ops.ceil32(cout)
    xd = nhwc(pad_c(x, cip))
    wd, bd = dev(w).requires_grad_(True), dev(b).requires_grad_(True)
    monkeypatch.setattr(ops, "PROFILE", [])
    y = ops.conv2d(xd, wd, bd, None, up=up)
    (y * nhwc(pad_c(gy, cop))).sum().backward()
    kinds = [r[0] for r in ops.PROFILE]
    # even-height, non-upsampled shapes take the 2-D F(3x3,2x2) form -- by default with the f32 products on the bf16 MFMA
    # (conv_wgrad_x6.hip) --, the others the 1-D F(3,2) form
    two_d = Ho >= 2                                            # (all the shapes here are powers of two)
    assert kinds.count("wgrad_wino2x6" if two_d else "wgrad_wino") == 1 and "wgrad" not in kinds, kinds
    close(wd.grad, wr.grad)
    close(bd.grad, br.grad)
    if two_d and not up:                                       # ... the f32-MFMA 2-D form (ADM_BF16X6=0) on the same problem
        monkeypatch.setattr(ops, "BF16X6", False)
        wd1, bd1 = dev(w).requires_grad_(True), dev(b).requires_grad_(True)
        monkeypatch.setattr(ops, "PROFILE", [])
        y1 = ops.conv2d(xd, wd1, bd1, None, up=up)
        (y1 * nhwc(pad_c(gy, cop))).sum().backward()
        assert [r[0] for r in ops.PROFILE].count("wgrad_wino2") == 1
        close(wd1.grad, wr.grad)
        close(bd1.grad, br.grad)
    monkeypatch.setattr(ops, "WINOGRAD2D", False)              # ... and the 1-D form
    wd2, bd2 = dev(w).requires_grad_(True), dev(b).requires_grad_(True)
    monkeypatch.setattr(ops, "PROFILE", [])
    y2 = ops.conv2d(xd, wd2, bd2, None, up=up)
    (y2 * nhwc(pad_c(gy, cop))).sum().backward()
    assert [r[0] for r in ops.PROFILE].count("wgrad_wino") == 1
    close(wd2.grad, wr.grad)
    close(bd2.grad, br.grad)


def test_linear_split_k_is_deterministic(ops):
    B, cin, cout = 7, 768, 768        # the embedding / affine Linear shape: split-K path
    from adm_amd import hip
    assert hip.lib().adm_conv_splitk(B, cout, cin) > 1
    x = fill.hash_tensor((B, cin), "skx", 1.0)
    w = fill.hash_tensor((cout, cin), "skw", 0.05)
    b = fill.hash_tensor((cout,), "skb", 0.1)
    r = fill.hash_tensor((B, cout), "skr", 1.0)
    y = ops.linear(dev(x), dev(w), dev(b), dev(r))
    close(y, x @ w.t() + b + r)
    assert torch.equal(y, ops.linear(dev(x), dev(w), dev(b), dev(r)))


def test_linear_and_qkv_permutation(ops):
    B, cin, heads = 5, 128, 2
    x = fill.hash_tensor((B, cin), "lx", 1.0)
    w = fill.hash_tensor((3 * 64 * heads, cin, 1, 1), "lw", 0.1)
    b = fill.hash_tensor((3 * 64 * heads,), "lb", 0.1)
    y_ref = x @ w.reshape(w.shape[0], cin).t() + b
    y = ops.linear(dev(x), dev(w.reshape(w.shape[0], cin)), dev(b))
    close(y, y_ref)
    # qkv=True: output channel (head, {q,k,v}, c) must equal reference channel (head, c, {q,k,v})
    yq = ops.conv2d(dev(x).reshape(B, 1, 1, cin), dev(w), dev(b), qkv=True).reshape(B, heads, 3, 64).cpu()
    close(yq, y_ref.reshape(B, heads, 64, 3).permute(0, 1, 3, 2))


@pytest.mark.parametrize("C,H,with_ss,silu", [(192, 32, True, True), (384, 16, False, True), (576, 8, True, True),
                                              (768, 4, False, False), (64, 8, True, True), (96, 16, False, True),
                                              (32, 4, False, True)])
def test_group_norm_act(ops, C, H, with_ss, silu):
    B = 3
    G = min(32, C // 4)
    x = fill.hash_tensor((B, C, H, H), f"gx{C}", 2.0) + 0.3
    gam = 1 + fill.hash_tensor((C,), f"gg{C}", 0.2)
    bet = fill.hash_tensor((C,), f"gb{C}", 0.1)
    ss = fill.hash_tensor((B, 2 * C), f"gs{C}", 0.5)
    gy = fill.hash_tensor((B, C, H, H), f"gy{C}", 1.0)
    xr, gr, br, sr = [t.clone().requires_grad_(True) for t in (x, gam, bet, ss)]
    z = F.group_norm(xr, G, gr, br, 1e-5)
    if with_ss:
        sc, sh = sr[:, :, None, None].chunk(2, dim=1)
        z = torch.addcmul(sh, z, sc + 1)
    y_ref = F.silu(z) if silu else z
    (y_ref * gy).sum().backward()
    xd = nhwc(x).requires_grad_(True)
    gd, bd = dev(gam).requires_grad_(True), dev(bet).requires_grad_(True)
    sd = dev(ss).requires_grad_(True) if with_ss else None
    y = ops.group_norm_act(xd, gd, bd, sd, silu=silu)
    close(nchw(y), y_ref)
    (y * nhwc(gy)).sum().backward()
    close(nchw(xd.grad), xr.grad)
    close(gd.grad, gr.grad)
    close(bd.grad, br.grad)
    if with_ss:
        close(sd.grad, sr.grad)
    # batch-broadcast scale/shift (the sampling call pattern: embedding at batch 1)
    if with_ss:
        y1 = ops.group_norm_act(nhwc(x), dev(gam), dev(bet), dev(ss[:1]), silu=silu)
        sc, sh = ss[:1, :, None, None].chunk(2, dim=1)
        z1 = torch.addcmul(sh, F.group_norm(x, G, gam, bet, 1e-5), sc + 1)
        close(nchw(y1), F.silu(z1) if silu else z1)


def test_dropout_mask_is_consistent(ops):
    B, C, H, p = 4, 64, 16, 0.1
    x = nhwc(fill.hash_tensor((B, C, H, H), "dx", 1.0)).requires_grad_(True)
    g, b = dev(torch.ones(C)), dev(torch.zeros(C))
    y0 = ops.group_norm_act(x, g, b, None, silu=True)
    y1 = ops.group_norm_act(x, g, b, None, silu=True, drop_p=p, seed=1234)
    y2 = ops.group_norm_act(x, g, b, None, silu=True, drop_p=p, seed=1234)
    y3 = ops.group_norm_act(x, g, b, None, silu=True, drop_p=p, seed=99)
    assert torch.equal(y1, y2) and not torch.equal(y1, y3)
    kept = (y1 != 0) | (y0 == 0)
    frac = 1 - kept.float().mean().item()
    assert abs(frac - p) < 0.01, frac
    close(y1[kept], (y0 / (1 - p))[kept])
    y1.sum().backward()       # gradient must use the same mask: zero where dropped
    gx = x.grad.clone()
    x.grad = None
    # finite-difference-free check: the gradient of sum(y) w.r.t. the pre-dropout activations is mask/(1-p);
    # compare against autograd through the unfused composition with the recovered mask
    xr = x.detach().cpu().permute(0, 3, 1, 2).clone().requires_grad_(True)
    mask = kept.cpu().permute(0, 3, 1, 2).float() / (1 - p)
    (F.silu(F.group_norm(xr, 16, torch.ones(C), torch.zeros(C), 1e-5)) * mask).sum().backward()
    close(nchw(gx), xr.grad)


@pytest.mark.parametrize("L,heads", [(16, 6), (64, 6), (256, 6), (64, 1), (256, 2), (1024, 2), (576, 1)])   # > 256: chunked, online softmax
def test_attention(ops, L, heads):
    B, h, C = 2, int(math.isqrt(L)), 64 * heads
    qkv = fill.hash_tensor((B, 3 * C, h, h), f"attn{L}.{heads}", 1.5).requires_grad_(True)
    a_ref = unet_ref.attention_core(qkv, heads)
    gy = fill.hash_tensor(a_ref.shape, f"ag{L}", 1.0)
    (a_ref * gy).sum().backward()
    # reference channel (head, c, j) -> packed (head, j, c)
    to_packed = lambda t: t.reshape(B, heads, 64, 3, h, h).permute(0, 1, 3, 2, 4, 5).reshape(B, 3 * C, h, h)
    from_packed = lambda t: t.reshape(B, heads, 3, 64, h, h).permute(0, 1, 3, 2, 4, 5).reshape(B, 3 * C, h, h)
    qd = nhwc(to_packed(qkv.detach())).requires_grad_(True)
    a = ops.attention(qd, heads)
    close(nchw(a), a_ref)
    (a * nhwc(gy)).sum().backward()
    close(from_packed(nchw(qd.grad)), qkv.grad)


@pytest.mark.parametrize("L,heads,scale", [(256, 6, 1.5), (64, 2, 1.5), (256, 1, 6.0), (1024, 1, 1.5), (1024, 2, 4.0), (576, 1, 1.5)])
def test_attention_forward_fp16_format(ops, monkeypatch, L, heads, scale):
    """The attention forward on the fp16 split format (attention_h3.hip: three fp16 MFMAs per f32 product in both matrix products; V
    transposed in LDS with the keys in the accumulator layout's order) against the oracle's attention core and against an fp64
    softmax(q k^T / 8) v: peaked softmaxes (scale 6: logits up to a few hundred), exact and 8x loose bounds of |qkv|; error at the f32 kernel's level; the
    backward on the same format; L = 1024 (the latent configs' 32x32 level) goes through 256-key chunks with the online softmax;
    L = 576 has no fp16 kernel and must fall back."""
    B, h, C = 2, int(math.isqrt(L)), 64 * heads
    qkv = fill.hash_tensor((B, 3 * C, h, h), f"attnh{L}.{heads}", scale).requires_grad_(True)
    a_ref = unet_ref.attention_core(qkv, heads)
    gy = fill.hash_tensor(a_ref.shape, f"agh{L}", 1.0)
    (a_ref * gy).sum().backward()
    to_packed = lambda t: t.reshape(B, heads, 64, 3, h, h).permute(0, 1, 3, 2, 4, 5).reshape(B, 3 * C, h, h)
    from_packed = lambda t: t.reshape(B, heads, 3, 64, h, h).permute(0, 1, 3, 2, 4, 5).reshape(B, 3 * C, h, h)
    q64 = qkv.detach().double().reshape(B * heads, 64, 3, L)
    w64 = torch.softmax(torch.einsum("ncq,nck->nqk", q64[:, :, 0], q64[:, :, 1] / 8.0), dim=2)
    a64 = torch.einsum("nqk,nck->ncq", w64, q64[:, :, 2]).reshape(B, C, h, h)
    q64g = qkv.detach().double().clone().requires_grad_(True)
    qq = q64g.reshape(B * heads, 64, 3, L)
    wg = torch.softmax(torch.einsum("ncq,nck->nqk", qq[:, :, 0], qq[:, :, 1] / 8.0), dim=2)
    (torch.einsum("nqk,nck->ncq", wg, qq[:, :, 2]).reshape(B, C, h, h) * gy.double()).sum().backward()
    g64 = q64g.grad
    errs, gerr = {}, {}
    for mode, loose in (("f32", 1.0), ("h3", 1.0), ("h3", 8.0)):
        monkeypatch.setattr(ops, "ATTN_H3", mode == "h3")
        qd = nhwc(to_packed(qkv.detach())).requires_grad_(True)
        qd._adm_amax = _amax(qd) * loose
        monkeypatch.setattr(ops, "PROFILE", [])
        a = ops.attention(qd, heads)
        kinds = [k[0] for k in ops.PROFILE]
        assert kinds == (["attnh3"] if (mode == "h3" and (L in (32, 64, 128, 256) or L % 256 == 0)) else ["attn"]), kinds
        close(nchw(a), a_ref)
        errs[(mode, loose)] = float((nchw(a).double() - a64).abs().max()) / float(a64.abs().max())
        # the backward on the same format needs the bound of dout as well (in the model: the proj conv's data gradient leaves it)
        gyd = nhwc(gy)
        monkeypatch.setattr(ops, "_get_amax", (lambda t, loose=loose: _amax(t) * loose) if mode == "h3" else (lambda t: None))
        monkeypatch.setattr(ops, "PROFILE", [])
        (a * gyd).sum().backward()
        kinds = [k[0] for k in ops.PROFILE]
        assert kinds == (["attnh3"] if (mode == "h3" and (L in (32, 64, 128, 256) or L % 256 == 0)) else ["attn"]), kinds
        close(from_packed(nchw(qd.grad)), qkv.grad)
        gerr[(mode, loose)] = float((from_packed(nchw(qd.grad)).double() - g64).abs().max()) / float(g64.abs().max())
    print(f"attention forward error / max|out| vs fp64: f32 MFMA {errs[('f32', 1.0)]:.2e}, fp16 format {errs[('h3', 1.0)]:.2e} (bound x 8: {errs[('h3', 8.0)]:.2e})")
    assert errs[("h3", 1.0)] <= max(3.0 * errs[("f32", 1.0)], 5e-7) and errs[("h3", 8.0)] <= max(4.0 * errs[("f32", 1.0)], 1e-6), errs
    print(f"attention backward error / max|dqkv| vs fp64: f32 MFMA {gerr[('f32', 1.0)]:.2e}, fp16 format {gerr[('h3', 1.0)]:.2e} (bounds x 8: {gerr[('h3', 8.0)]:.2e})")
    assert gerr[("h3", 1.0)] <= max(3.0 * gerr[("f32", 1.0)], 1e-6) and gerr[("h3", 8.0)] <= max(4.0 * gerr[("f32", 1.0)], 2e-6), gerr


def test_resample_concat_silu_posemb(ops):
    x = fill.hash_tensor((2, 64, 8, 8), "rs", 1.0).requires_grad_(True)
    gy_d = fill.hash_tensor((2, 64, 4, 4), "rsd", 1.0)
    gy_u = fill.hash_tensor((2, 64, 16, 16), "rsu", 1.0)
    yd = F.avg_pool2d(x, 2)
    yu = F.interpolate(x, scale_factor=2, mode="nearest")
    ((yd * gy_d).sum() + (yu * gy_u).sum()).backward()
    xd = nhwc(x.detach()).requires_grad_(True)
    d, u = ops.downsample2x(xd), ops.upsample2x(xd)
    close(nchw(d), yd); close(nchw(u), yu)
    ((d * nhwc(gy_d)).sum() + (u * nhwc(gy_u)).sum()).backward()
    close(nchw(xd.grad), x.grad)
    a = nhwc(fill.hash_tensor((2, 64, 4, 4), "ca", 1.0)).requires_grad_(True)
    b = nhwc(fill.hash_tensor((2, 32, 4, 4), "cb", 1.0)).requires_grad_(True)
    c = ops.concat_channels(a, b, 0.75)
    close(c, torch.cat([a, 0.75 * b], dim=-1))
    w = dev(fill.hash_tensor(c.shape, "cw", 1.0))
    (c * w).sum().backward()
    close(a.grad, w[..., :64]); close(b.grad, 0.75 * w[..., 64:])
    s = dev(fill.hash_tensor((7, 33), "si", 3.0)).requires_grad_(True)
    y = ops.silu(s)
    close(y, F.silu(s.detach().cpu()))
    y.sum().backward()
    sr = s.detach().cpu().requires_grad_(True)
    F.silu(sr).sum().backward()
    close(s.grad, sr.grad)
    t = torch.tensor([1e-4, 0.5, 1.0]).log()
    close(ops.pos_embedding(dev(t), 192), unet_ref.positional_embedding(t, 192))


def test_spatial_att_gate(ops):
    B, C, H = 3, 64, 4
    sd = {k: fill.fill_value("sa." + k, s) for k, s in {"map.weight": (1, C, 1, 1), "map.bias": (1,),
          "q_conv.weight": (1, 1, 1, 1), "q_conv.bias": (1,), "k_conv.weight": (1, 1, 1, 1), "k_conv.bias": (1,)}.items()}
    sd = {"sa." + k: v.requires_grad_(True) for k, v in sd.items()}
    h = fill.hash_tensor((B, C, H, H), "sah", 1.0).requires_grad_(True)
    xres = fill.hash_tensor((B, C, H, H), "sax", 1.0).requires_grad_(True)
    gy = fill.hash_tensor((B, C, H, H), "sag", 1.0)
    y_ref = unet_ref.spatial_att(sd, "sa", h) + xres
    (y_ref * gy).sum().backward()
    hd, xd = nhwc(h.detach()).requires_grad_(True), nhwc(xres.detach()).requires_grad_(True)
    mw, mb = dev(sd["sa.map.weight"].detach()).requires_grad_(True), dev(sd["sa.map.bias"].detach()).requires_grad_(True)
    qk = dev(torch.stack([sd["sa.q_conv.weight"].detach().reshape(()), sd["sa.q_conv.bias"].detach().reshape(()),
                          sd["sa.k_conv.weight"].detach().reshape(()), sd["sa.k_conv.bias"].detach().reshape(())]))
    qk.requires_grad_(True)
    att = ops.conv2d(hd, mw, mb)
    y = ops.spatial_att_gate(att, qk, hd, xd)
    close(nchw(y), y_ref)
    (y * nhwc(gy)).sum().backward()
    close(nchw(hd.grad), h.grad)
    close(nchw(xd.grad), xres.grad)
    close(mw.grad, sd["sa.map.weight"].grad)
    want = torch.stack([sd["sa.q_conv.weight"].grad.reshape(()), sd["sa.q_conv.bias"].grad.reshape(()),
                        sd["sa.k_conv.weight"].grad.reshape(()), sd["sa.k_conv.bias"].grad.reshape(())])
    close(qk.grad, want)


def test_schedule_kernels(ops):
    from oracle import ddm_ref
    B = 4
    x0 = fill.hash_tensor((B, 3, 32, 32), "x0", 1.0)
    noise = fill.hash_tensor((B, 3, 32, 32), "noise", 1.7)
    t = torch.tensor([0.23, 0.81, 1e-4, 0.999])
    for sched_i, sched in enumerate(("const", "const_2")):
        close(ops.q_sample(dev(x0), dev(noise), dev(t), sched_i), ddm_ref.q_sample(sched, x0, noise, t, -x0))
        cp = fill.hash_tensor((B, 3, 32, 32), "cp", 1.0).requires_grad_(True)
        npd = fill.hash_tensor((B, 3, 32, 32), "np", 1.0).requires_grad_(True)
        w1, w2 = ddm_ref.loss_weights(sched, t, 1e-4)
        loss_ref = (w1 * ((cp + x0) ** 2).sum([1, 2, 3]) + w2 * ((npd - noise) ** 2).sum([1, 2, 3])).sum() / B
        loss_ref.backward()
        cd, nd = dev(cp.detach()).requires_grad_(True), dev(npd.detach()).requires_grad_(True)
        loss, per = ops.ddm_loss(cd, nd, dev(x0), dev(noise), dev(torch.stack([w1, w2], 1)))
        close(loss, loss_ref)
        loss.backward()
        close(cd.grad, cp.grad); close(nd.grad, npd.grad)
        # one fp64 sampler update
        x = fill.hash_tensor((B, 3, 32, 32), "xs", 1.0, torch.float64)
        g = (lambda v: math.sqrt(v)) if sched == "const" else (lambda v: v)
        tc, tn = 0.6, 0.45
        x0e = x - cp.detach().double() * tc - npd.detach().double() * g(tc)
        if sched == "const":
            x0e = x0e.clamp(-1, 1)
        want = x0e + cp.detach().double() * tn + npd.detach().double() * g(tn)
        got = ops.sampler_step(dev(x), dev(cp.detach()), dev(npd.detach()), tc, tn, sched_i, sched == "const", 1.0, False)
        assert got.dtype == torch.float64
        close(got, want, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ fp16 split format (round 3)
def _amax(t):
    from adm_amd import ops as _ops
    return _ops.amax_vector(t)      # a bound vector (include/adm_hip.h): max |t| in slot 0


@pytest.mark.parametrize("B,cin,cout,H,up", [(8, 64, 96, 32, False), (4, 192, 192, 16, False), (8, 96, 64, 16, True), (2, 32, 64, 8, False),
                                             (128, 384, 384, 4, False), (4, 64, 160, 8, True), (32, 64, 256, 32, False)])
@pytest.mark.parametrize("wide", [-1, 1, 3])
def test_conv_h3_forward_vs_torch(ops, monkeypatch, request, B, cin, cout, H, up, wide):
    """The 3x3 forward on THREE fp16 products per f32 product (adm_conv_fwd_wino2d_h3) against F.conv2d: plain, with the fused nearest
    x2, with bias and residual, on the split-K shapes of the 4x4 maps -- and with a LOOSE bound (8 x the true maximum: the bound only
    has to be an upper bound).  The launch record proves the format."""
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    from adm_amd import hip as _hip
    old_wide = _hip.lib().adm_wino2d_h3_wide(wide)     # 1 / 3: the 128- / 96-cout workgroups (eight / six consumer waves) on every shape; -1: per launch
    request.addfinalizer(lambda: _hip.lib().adm_wino2d_h3_wide(old_wide))
    x = fill.hash_tensor((B, cin, H, H), f"h3x{cin}{H}", 1.0)
    w = fill.hash_tensor((cout, cin, 3, 3), f"h3w{cin}{cout}", 1.0 / math.sqrt(cin * 9))
    b = fill.hash_tensor((cout,), f"h3b{cout}", 0.5)
    Ho = 2 * H if up else H
    r = fill.hash_tensor((B, cout, Ho, Ho), f"h3r{cout}{H}", 1.0)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    want = F.conv2d(xin, w, b, padding=1) + r
    wd, bd = dev(w), dev(b)
    for loose in (1.0, 8.0):
        monkeypatch.setattr(ops, "PROFILE", [])
        y = ops.conv2d(nhwc(x), wd, bd, nhwc(r), up=up, amax=_amax(dev(x)) * loose)
        assert [k[0] for k in ops.PROFILE] == ["wino2h3"], [k[0] for k in ops.PROFILE]
        close(nchw(y)[:, :cout], want)
    assert wd._adm_packed.w2fh is not None
    monkeypatch.setattr(ops, "FP16X3", False)          # the switch: same call, bf16 format
    monkeypatch.setattr(ops, "PROFILE", [])
    y6 = ops.conv2d(nhwc(x), wd, bd, nhwc(r), up=up, amax=_amax(dev(x)))
    assert [k[0] for k in ops.PROFILE] == ["wino2x6"]
    close(nchw(y6)[:, :cout], want)


@pytest.mark.parametrize("B,cin,cout,H,ks,up,det", [(8, 64, 96, 32, 3, False, False), (4, 192, 192, 16, 3, False, True), (8, 96, 64, 16, 3, True, False),
                                                    (2, 32, 64, 8, 3, False, False), (128, 384, 384, 4, 3, False, False),
                                                    (8, 384, 384, 32, 1, False, False), (9, 192, 96, 32, 1, False, True),
                                                    (4, 64, 160, 16, 3, True, False), (33, 96, 224, 16, 1, False, False)])
@pytest.mark.parametrize("blocks", [-1, 1, 2])
def test_conv_h3_weight_gradient_vs_torch(ops, monkeypatch, request, B, cin, cout, H, ks, up, det, blocks):
    """Weight and bias gradients on the fp16 format (conv_wgrad_x6.hip FMT 1: adm_conv_wgrad_x6_h3 / adm_gemm_wgrad_x6_h3) against
    autograd's on the CPU: 3x3 (plain, fused nearest x2, split over many workgroups, the deterministic workspace mode) and 1x1; the
    bounds of x and dy are the true maxima times 1 and times 8 (only an upper bound is needed); the launch record proves the format;
    the error against an fp64 gradient stays at the six-bf16 form's."""
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    monkeypatch.setattr(ops, "DETERMINISTIC", det)
    from adm_amd import hip as _hip
    old_blocks = _hip.lib().adm_wgrad_h3_blocks(blocks)      # -1: 128 couts per workgroup (sixteen waves) for the 3x3 form where > 64 couts; 2: also for the 1x1 form; 1: 64
    request.addfinalizer(lambda: _hip.lib().adm_wgrad_h3_blocks(old_blocks))
    x = fill.hash_tensor((B, cin, H, H), f"hwx{cin}{H}", 1.0)
    w = fill.hash_tensor((cout, cin, ks, ks), f"hww{cin}{cout}", 1.0 / math.sqrt(cin * ks * ks))
    b = fill.hash_tensor((cout,), f"hwb{cout}", 0.5)
    Ho = 2 * H if up else H
    gy = fill.hash_tensor((B, cout, Ho, Ho), f"hwg{cout}{H}", 3.0)
    wr, br = w.clone().double().requires_grad_(True), b.clone().double().requires_grad_(True)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    (F.conv2d(xin.double(), wr, br, padding=ks // 2) * gy.double()).sum().backward()
    scale = float(F.conv2d(xin.abs().double().transpose(0, 1), gy.abs().double().transpose(0, 1), padding=ks // 2).max())   # max sum |x dy|
    errs = {}
    for mode, loose in (("h3", 1.0), ("h3", 8.0), ("x6", 1.0)):
        monkeypatch.setattr(ops, "H3_WGRAD", mode == "h3")
        monkeypatch.setattr(ops, "_get_amax", lambda t, loose=loose: _amax(t) * loose)       # dy's bound (in a model: its producer's)
        wd, bd = dev(w).requires_grad_(True), dev(b).requires_grad_(True)
        y = ops.conv2d(nhwc(x), wd, bd, up=up, amax=_amax(dev(x)) * loose)
        monkeypatch.setattr(ops, "PROFILE", [])
        (y * nhwc(gy)).sum().backward()
        kinds = [k[0] for k in ops.PROFILE]
        tag = ("wgrad_wino2" if ks == 3 else "wgrad_gemm") + mode
        assert kinds.count(tag) == 1, (tag, kinds)
        close(wd.grad, wr.grad.float())
        close(bd.grad, br.grad.float())
        errs[(mode, loose)] = float((wd.grad.double().cpu() - wr.grad).abs().max()) / scale
    print(f"dW error / max sum|x dy|: three fp16 {errs[('h3', 1.0)]:.3e} (bound x 8: {errs[('h3', 8.0)]:.3e}), six bf16 {errs[('x6', 1.0)]:.3e}")
    assert errs[("h3", 1.0)] <= max(2.0 * errs[("x6", 1.0)], 2e-7) and errs[("h3", 8.0)] <= max(4.0 * errs[("x6", 1.0)], 4e-7), errs


@pytest.mark.parametrize("B,cin,cout,H,qkv,with_res", [(8, 384, 384, 32, False, True), (9, 192, 384, 31, False, False), (8, 384, 1152, 32, True, False),
                                                        (32, 768, 128, 16, False, True), (8, 576, 192, 32, False, True), (8, 192, 576, 32, False, False)])
def test_conv1x1_h3_forward_backward(ops, monkeypatch, B, cin, cout, H, qkv, with_res):
    """1x1 convs on the fp16 format (conv_gemm_x6.hip FMT 1: adm_gemm_x6_h3): forward (bias, residual, the qkv row permutation, ragged
    pixel counts), data gradient and -- through conv_wgrad_x6.hip MODE 1 FMT 1 -- weight / bias gradients against F.conv2d on the CPU;
    the launch record proves the format; the bound the epilogue leaves on the output is EXACTLY max |y|; error vs fp64 at the
    six-bf16 form's."""
    x = fill.hash_tensor((B, cin, H, H), f"g3x{cin}{cout}", 1.0)
    w = fill.hash_tensor((cout, cin, 1, 1), f"g3w{cin}{cout}", 1.0 / math.sqrt(cin))
    b = fill.hash_tensor((cout,), f"g3b{cin}{cout}", 0.5)
    r = fill.hash_tensor((B, cout, H, H), f"g3r{cin}{cout}", 1.0)
    gy = fill.hash_tensor((B, cout, H, H), f"g3g{cin}{cout}", 2.0)
    xr, wr, br = [t.double().clone().requires_grad_(True) for t in (x, w, b)]
    y_ref = F.conv2d(xr, wr, br) + (r.double() if with_res else 0)
    (y_ref * gy.double()).sum().backward()
    s_y = float(F.conv2d(x.double().abs(), w.double().abs()).max())
    errs = {}
    for mode in ("h3", "x6"):
        monkeypatch.setattr(ops, "H3_GEMM", mode == "h3")
        monkeypatch.setattr(ops, "_get_amax", (lambda t: _amax(t) * 2.0) if mode == "h3" else (lambda t: None))      # dy's bound, loose by 2
        xd = nhwc(x).requires_grad_(True)
        wd, bd = torch.nn.Parameter(dev(w)), torch.nn.Parameter(dev(b))
        monkeypatch.setattr(ops, "PROFILE", [])
        y = ops.conv2d(xd, wd, bd, nhwc(r) if with_res else None, qkv=qkv, amax=_amax(dev(x)))
        kinds = [k[0] for k in ops.PROFILE]
        assert kinds == ["gemm" + mode], kinds
        if mode == "h3":
            assert float(y._adm_amax.max()) == float(y.detach().abs().max())       # the epilogue's bound of the output
        yn = nchw(y)
        if qkv:
            heads = cout // 192
            yn = yn.reshape(B, heads, 3, 64, H, H).permute(0, 1, 3, 2, 4, 5).reshape(B, cout, H, H)
        close(yn, y_ref.detach().float())
        errs[mode] = float((yn.double() - y_ref.detach()).abs().max()) / s_y
        if qkv:
            continue
        monkeypatch.setattr(ops, "PROFILE", [])
        (y * nhwc(gy)).sum().backward()
        kinds = [k[0] for k in ops.PROFILE]
        assert kinds.count("gemm" + mode) == (1 if cin >= 128 else 0) and kinds.count("wgrad_gemm" + mode) == 1, kinds
        close(nchw(xd.grad), xr.grad.float())
        close(wd.grad, wr.grad.float())
        close(bd.grad, br.grad.float())
    print(f"1x1 forward error / max sum|ab|: three fp16 {errs['h3']:.3e}, six bf16 {errs['x6']:.3e}")
    assert errs["h3"] <= max(2.0 * errs["x6"], 2e-7), errs


def test_conv_h3_error_vs_fp64(ops, monkeypatch):
    """Accuracy of the three-fp16-product form against an fp64 convolution, next to the six-bf16-product form and the f32 MFMA kernel,
    relative to max sum |a b|: zero-mean data, all-positive data (no cancellation), heavy-tailed activations (log-normal magnitudes over
    ~2^17) and a single huge outlier that sets the scale for everybody else."""
    B, C, H = 4, 384, 16
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    g = torch.Generator().manual_seed(3)
    base = fill.hash_tensor((B, C, H, H), "h64x", 1.0)
    cases = {"zero-mean": base, "positive": base.abs(),
             "heavy-tailed": base * torch.exp(torch.randn(base.shape, generator=g) * 2.5),
             "outlier": base.clone()}
    cases["outlier"][0, 0, 0, 0] = 3.0e4
    w = fill.hash_tensor((C, C, 3, 3), "h64w", 0.02)
    for name, x in cases.items():
        ww = w.abs() if name == "positive" else w
        ref = F.conv2d(x.double(), ww.double(), padding=1)
        scale = float(F.conv2d(x.double().abs(), ww.double().abs(), padding=1).max())
        err = {}
        for mode in ("f32", "x6", "h3"):
            monkeypatch.setattr(ops, "BF16X6", mode != "f32")
            monkeypatch.setattr(ops, "FP16X3", mode == "h3")
            y = ops.conv2d(nhwc(x), dev(ww), None, amax=_amax(dev(x)) if mode == "h3" else None)
            err[mode] = float((nchw(y).double() - ref).abs().max()) / scale
        print(f"{name}: max|err| / max sum|ab|: f32 MFMA {err['f32']:.3e}, six bf16 {err['x6']:.3e}, three fp16 {err['h3']:.3e}")
        assert err["h3"] <= max(1.5 * err["f32"], 2e-7), (name, err)


def test_group_norm_writes_the_maximum_for_its_consumer(ops, monkeypatch):
    """group_norm_act(..., to_conv=True) hands max |y| to the conv (a device float raised by the same kernel): exact, for the
    register-resident small-map kernels and the multi-pass large-map path, with dropout and scale/shift; the 2x2-mean resampling keeps
    the bound; a UNet block's convs then run on the fp16 format."""
    for B, C, H in ((3, 192, 32), (4, 384, 16), (2, 384, 4), (2, 64, 8)):
        x = dev(fill.hash_tensor((B, H, H, C), f"gam{C}{H}", 2.0) + 0.3)
        gam, bet = dev(1 + fill.hash_tensor((C,), "gamg", 0.2)), dev(fill.hash_tensor((C,), "gamb", 0.1))
        ss = dev(fill.hash_tensor((B, 2 * C), "gams", 0.5))
        for kw in (dict(), dict(drop_p=0.1, seed=7)):
            y = ops.group_norm_act(x, gam, bet, ss, silu=True, to_conv=True, **kw)
            assert hasattr(y, "_adm_amax"), "no maximum attached"
            assert y._adm_amax.numel() == ops.AMAX_FLOATS              # a bound vector: the bound is the maximum of its slots
            assert float(y._adm_amax.max()) == float(y.abs().max()), (B, C, H, kw, float(y._adm_amax.max()), float(y.abs().max()))
            assert ops.downsample2x(y)._adm_amax is y._adm_amax
        y0 = ops.group_norm_act(x, gam, bet, ss, silu=True)           # not promised to a conv: no maximum
        assert not hasattr(y0, "_adm_amax")
    w = dev(fill.hash_tensor((192, 192, 3, 3), "gamw", 0.03))
    x = dev(fill.hash_tensor((8, 16, 16, 192), "gamx", 1.0))
    gam, bet = dev(torch.ones(192)), dev(torch.zeros(192))
    monkeypatch.setattr(ops, "PROFILE", [])
    ops.conv2d(ops.group_norm_act(x, gam, bet, None, silu=True, to_conv=True), w, None)
    assert "wino2h3" in [k[0] for k in ops.PROFILE]


def test_conv_h3_weights_follow_repack_all(ops, monkeypatch):
    """The fp16 images of the Winograd operands are refreshed by the one-launch repack table, bit for bit as adm_split2_f16 would."""
    from adm_amd import hip as _hip
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    x = fill.hash_tensor((2, 64, 8, 8), "h3rpx", 1.0)
    w = torch.nn.Parameter(dev(fill.hash_tensor((96, 64, 3, 3), "h3rpw", 0.05)))
    am = _amax(dev(x))
    y0 = ops.conv2d(nhwc(x), w, None, amax=am)
    pk = w._adm_packed
    assert pk.w2fh is not None
    assert pk.w2f6 is None and pk.w2bh is None and pk.w2b6 is None      # only the image that ran is built (and repacked every step)
    with torch.no_grad():
        w.data.mul_(1.5).add_(0.01)
    ops.repack_all()
    assert w._adm_packed is pk
    y1 = ops.conv2d(nhwc(x), w, None, amax=am)
    close(nchw(y1)[:, :96], F.conv2d(x, w.detach().cpu(), padding=1))
    assert not torch.equal(y0, y1)
    w2f, w2b = torch.empty((16, 96, 64), device=w.device), torch.empty((16, 64, 96), device=w.device)
    _hip.call("adm_pack_weight_wino2d", w.detach().data_ptr(), w2f.data_ptr(), w2b.data_ptr(), 96, 64, 96, 64)
    want = torch.empty_like(pk.w2fh)
    flag = torch.zeros(1, dtype=torch.int32, device=w.device)
    _hip.call("adm_split2_f16", w2f.data_ptr(), want.data_ptr(), 96, 64, ops.H3_WSCALE, flag.data_ptr())
    assert torch.equal(want.view(torch.int16), pk.w2fh.view(torch.int16)) and int(flag) == 0
    big = torch.full((16, 32, 32), 40.0, device=w.device)             # 40 * 2^11 leaves the fp16 range: the flag goes up
    _hip.call("adm_split2_f16", big.data_ptr(), torch.empty((16, 2, 32, 32), device=w.device, dtype=torch.float16).data_ptr(), 32, 32,
              ops.H3_WSCALE, flag.data_ptr())
    assert int(flag) == 1


def test_every_weight_image_follows_repack_all(ops, monkeypatch):
    """Every derived weight image a layer can hold -- both directions, 3x3 and 1x1, f32 planes, bf16 splits and fp16 images -- is built
    on first use by forward and backward under the setting that needs it, and after an in-place change of the weights is refreshed by
    the one launch of ops.repack_all() bit for bit as the per-layer pack / split kernels produce it."""
    from adm_amd import hip as _hip
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    monkeypatch.setattr(ops, "GEMM_X6_MIN_M", 1)
    monkeypatch.setattr(ops, "WINOGRAD", True)
    monkeypatch.setattr(ops, "_pack_registry", {})           # the table of this test holds its own layers only ...
    monkeypatch.setattr(ops, "_pack_table", None)
    monkeypatch.setattr(ops, "_h3_flag", None)               # ... and raises a flag of its own
    images = ("wf", "wb", "w2f", "w2b", "w2f6", "w2b6", "w2fh", "w2bh", "g6f", "g6b", "g6fh", "g6bh")
    x3, g3 = fill.hash_tensor((2, 64, 8, 8), "evx3", 1.0), fill.hash_tensor((2, 96, 8, 8), "evg3", 1.0)
    x1, g1 = fill.hash_tensor((2, 128, 8, 8), "evx1", 1.0), fill.hash_tensor((2, 128, 8, 8), "evg1", 1.0)
    layers = []
    for name, (w2d, x6, h3), want3, want1 in (("1d", (False, True, False), {"wf", "wb"}, None),
                                              ("f32", (True, False, False), {"w2f", "w2b"}, None),
                                              ("x6", (True, True, False), {"w2f6", "w2b6"}, {"g6f", "g6b"}),
                                              ("h3", (True, True, True), {"w2fh", "w2bh"}, {"g6fh", "g6bh"})):
        monkeypatch.setattr(ops, "WINOGRAD2D", w2d)
        monkeypatch.setattr(ops, "BF16X6", x6)
        monkeypatch.setattr(ops, "FP16X3", h3)
        for x, gy, shape, want in ((x3, g3, (96, 64, 3, 3), want3), (x1, g1, (128, 128, 1, 1), want1)):
            if want is None:
                continue
            w = torch.nn.Parameter(dev(fill.hash_tensor(shape, f"evw{name}{shape[-1]}", 0.05)))
            xd = nhwc(x).requires_grad_(True)
            y = ops.conv2d(xd, w, None, amax=_amax(xd) if h3 else None)
            if h3:      # the bound of dy, registered inside the backward pass as its producer would
                y.register_hook(lambda g: ops._reg_amax(g, _amax(g)))
            (y * nhwc(gy)).sum().backward()
            pk = w._adm_packed
            assert {n for n in images if getattr(pk, n) is not None} == want, (name, shape)
            layers.append((name, w, pk, want))
    with torch.no_grad():
        for _, w, _, _ in layers:
            w.data.mul_(1.5).add_(0.01)              # in place, as the optimiser kernel does (same storage)
    ops.repack_all()
    f32, bf16, f16 = torch.float32, torch.bfloat16, torch.float16
    gpu = layers[0][1].device
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)

    def made(shape, dtype, symbol, src, *args):
        t = torch.empty(shape, device=gpu, dtype=dtype)
        _hip.call(symbol, src.data_ptr(), t.data_ptr(), *args)
        return t

    for name, w, pk, want in layers:
        assert w._adm_packed is pk, name
        co, ci, ks = w.shape[0], w.shape[1], w.shape[-1]
        cop, cip = ops.ceil32(co), ops.ceil32(ci)
        ref = {"fwd": torch.empty((cop, ks * ks * cip), device=gpu), "bwd": torch.empty((cip, ks * ks * cop), device=gpu)}
        _hip.call("adm_pack_weight", w.data_ptr(), ref["fwd"].data_ptr(), ref["bwd"].data_ptr(), co, ci, ks, cop, cip, 0)
        if ks == 3:
            ref["wf"], ref["wb"] = torch.empty((4, cop, 3, cip), device=gpu), torch.empty((4, cip, 3, cop), device=gpu)
            _hip.call("adm_pack_weight_wino", w.data_ptr(), ref["wf"].data_ptr(), ref["wb"].data_ptr(), co, ci, cop, cip)
            ref["w2f"], ref["w2b"] = torch.empty((16, cop, cip), device=gpu), torch.empty((16, cip, cop), device=gpu)
            _hip.call("adm_pack_weight_wino2d", w.data_ptr(), ref["w2f"].data_ptr(), ref["w2b"].data_ptr(), co, ci, cop, cip)
            for d in "fb":
                src = ref["w2" + d]
                rows, cols = src.shape[1], src.shape[2]
                ref[f"w2{d}6"] = made((16, 3, rows, cols), bf16, "adm_split3_bf16", src, rows, cols)
                ref[f"w2{d}h"] = made((16, 2, rows, cols), f16, "adm_split2_f16", src, rows, cols, ops.H3_WSCALE, flag.data_ptr())
        else:
            for d, src in (("f", ref["fwd"]), ("b", ref["bwd"])):
                rows, cols = src.shape
                ref[f"g6{d}"] = made((3, rows, cols), bf16, "adm_split3_rows", src, rows, cols, cols)
                ref[f"g6{d}h"] = made((2, rows, cols), f16, "adm_split2_rows_f16", src, rows, cols, cols, ops.H3_WSCALE, flag.data_ptr())
        for n in ("fwd", "bwd") + tuple(sorted(want)):
            got, exp = getattr(pk, n), ref[n]
            assert got.shape == exp.shape and got.dtype == exp.dtype, (name, n, got.shape, exp.shape)
            assert torch.equal(got.view(torch.int32 if got.dtype == f32 else torch.int16), exp.view(torch.int32 if got.dtype == f32 else torch.int16)), (name, n)
    assert int(flag) == 0 and (ops._h3_flag is None or int(ops._h3_flag) == 0)

