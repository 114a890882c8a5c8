"""GPU: the opt-in bf16-MFMA contraction mode (BASELINE configs[2]).  No reference counterpart exists (every
reference config runs fp32), so the bar is the build's own: (1) against a torch reference whose OPERANDS are
rounded to bf16 the kernels must agree to fp32-accumulation accuracy (rtol 2e-4): that isolates the kernel from
the rounding; (2) against the un-rounded fp32 reference the error must stay at bf16 level (2e-2 of the output
scale); (3) end to end on the reduced UNet: <= 3e-2 of the output scale for outputs, cosine >= 0.999 for the
flattened gradient.  The storage mode at full width, GroupNorm -> conv with a residual, is held to bars A and B of
tests/test_hip_accuracy.py against fp64 of the values as stored; the direct kernels per tile form are in
tests/test_hip_bf16_accuracy.py."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import fill, unet_ref

import fp64ref
import gn_cases

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ops_bf16():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip, ops
    hip.lib()
    ops.set_compute_precision("bf16")
    yield ops
    ops.set_compute_precision("f32")


def r16(t):
    return t.to(torch.bfloat16).to(torch.float32)


# the last two: a residual per kernel size (the epilogues read it with their own indexing).  The ids of the earlier cases are kept.
_CONV_CASES = [(64, 128, 16, 3, False, False), (192, 192, 32, 3, False, False), (128, 64, 8, 1, False, False), (64, 64, 8, 3, True, False),
               (384, 96, 12, 3, False, False), (64, 3, 16, 3, False, False), (64, 96, 12, 3, False, True), (128, 192, 12, 1, False, True)]


@pytest.mark.parametrize("cin,cout,H,ks,up,with_res", _CONV_CASES,
                         ids=["-".join(str(v) for v in c[:5]) + ("-res" if c[5] else "") for c in _CONV_CASES])
def test_conv_bf16_forward_backward(ops_bf16, monkeypatch, cin, cout, H, ks, up, with_res):
    ops = ops_bf16
    B = 3
    x = fill.hash_tensor((B, cin, H, H), f"bx{cin}{cout}", 1.0)
    w = fill.hash_tensor((cout, cin, ks, ks), f"bw{cin}{cout}", 1.0 / math.sqrt(cin * ks * ks))
    b = fill.hash_tensor((cout,), f"bb{cin}{cout}", 0.5)
    Ho = 2 * H if up else H
    gy = fill.hash_tensor((B, cout, Ho, Ho), f"bg{cin}{cout}", 1.0)
    r = fill.hash_tensor((B, cout, Ho, Ho), f"br{cin}{cout}", 1.0) if with_res else None
    cop = ops.ceil32(cout)
    pad = lambda t, c: torch.cat([t, torch.zeros(t.shape[0], c - t.shape[1], *t.shape[2:])], 1) if c > t.shape[1] else t
    xd = pad(x, ops.ceil32(cin)).permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
    wd, bd = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    rd = pad(r, cop).permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True) if with_res else None
    names = []
    orig_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), orig_call(name, *a))[1])
    y = ops.conv2d(xd, wd, bd, rd, up=up)
    gyd = pad(gy, cop).permute(0, 2, 3, 1).contiguous().cuda()
    (y * gyd).sum().backward()
    yh = y.detach().cpu().permute(0, 3, 1, 2)[:, :cout]

    def ref(xx, ww, gg):
        xr, wr, br = xx.clone().requires_grad_(True), ww.clone().requires_grad_(True), b.clone().requires_grad_(True)
        xin = F.interpolate(xr, scale_factor=2, mode="nearest") if up else xr
        yr = F.conv2d(xin, wr, br, padding=ks // 2)
        if with_res:
            yr = yr + r
        return yr, xr, wr

    # (1) operands rounded exactly as the kernel rounds them.  dgrad rounds dy and w; wgrad rounds dy and x.
    yr, xr, wr = ref(r16(x), r16(w), gy)
    torch.testing.assert_close(yh, yr.detach(), rtol=2e-4, atol=2e-4 * float(yr.detach().abs().max()))
    yr.backward(r16(gy))
    y32, x32, w32 = ref(x, w, gy)
    y32.backward(gy)
    dxh = xd.grad.cpu().permute(0, 3, 1, 2)[:, :cin]
    if cop % 64 == 0:       # dgrad ran in bf16: forward and data gradient on the same entry point
        assert names.count("adm_conv_fwd_bf16") == 2, names
        torch.testing.assert_close(dxh, xr.grad, rtol=2e-4, atol=2e-4 * float(xr.grad.abs().max()))
    else:                   # dy has a channel count the bf16 kernel does not take: the data gradient ran on the f32 kernel, on the
        #                     un-rounded dy and w -- it meets the same fp32-accumulation tolerance against the UN-ROUNDED reference
        assert names.count("adm_conv_fwd_bf16") == 1, names
        torch.testing.assert_close(dxh, x32.grad, rtol=2e-4, atol=2e-4 * float(x32.grad.abs().max()))
    # (x is f32 here: the direct bf16 kernel, which rounds dy and x on load.  With bf16-STORED activations the 3x3 weight gradient
    #  runs on the split-bf16 Winograd kernel instead: test_wgrad_x6_bf16_activations_equal_f32_kernel_on_rounded_x)
    assert names.count("adm_conv_wgrad_bf16") == 1, names
    torch.testing.assert_close(wd.grad.cpu(), wr.grad, rtol=2e-4, atol=3e-4 * float(wr.grad.abs().max()))
    # (2) versus full fp32: bf16-level error only
    assert float((yh - y32.detach()).abs().max()) <= 2e-2 * float(y32.abs().max())
    assert float((wd.grad.cpu() - w32.grad).abs().max()) <= 2e-2 * float(w32.grad.abs().max())
    torch.testing.assert_close(bd.grad.cpu(), gy.sum(dim=(0, 2, 3)), rtol=1e-4, atol=1e-4 * float(gy.sum(dim=(0, 2, 3)).abs().max()))
    if with_res:            # the residual's gradient is dy itself
        assert torch.equal(rd.grad, gyd)


@pytest.mark.parametrize("B,cin,cout,H,W", [(1, 64, 64, 1, 2), (1, 64, 128, 2, 2), (2, 128, 64, 1, 1), (3, 64, 64, 3, 5)])
def test_conv_bf16_tiny_images(ops_bf16, B, cin, cout, H, W):
    """Edge cases of the bf16 forward / data-gradient / weight-gradient kernels: images smaller than the filter (the
    shifted buffer descriptor of the weight-gradient kernels must clamp at 0: round-1 fault, conv_wgrad_bf16.hip:51)."""
    ops = ops_bf16
    x = fill.hash_tensor((B, cin, H, W), f"tx{cin}{cout}{H}{W}", 1.0)
    w = fill.hash_tensor((cout, cin, 3, 3), f"tw{cin}{cout}", 1.0 / math.sqrt(cin * 9))
    gy = fill.hash_tensor((B, cout, H, W), f"tg{cin}{cout}{H}{W}", 1.0)
    xd = x.permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
    wd = w.cuda().requires_grad_(True)
    y = ops.conv2d(xd, wd, None, None)
    (y * gy.permute(0, 2, 3, 1).contiguous().cuda()).sum().backward()
    xr, wr = r16(x).requires_grad_(True), r16(w).requires_grad_(True)
    yr = F.conv2d(xr, wr, None, padding=1)
    yr.backward(r16(gy))
    torch.testing.assert_close(y.detach().cpu().permute(0, 3, 1, 2), yr.detach(), rtol=2e-4, atol=2e-4 * float(yr.abs().max()))
    torch.testing.assert_close(xd.grad.cpu().permute(0, 3, 1, 2), xr.grad, rtol=2e-4, atol=2e-4 * float(xr.grad.abs().max()))
    torch.testing.assert_close(wd.grad.cpu(), wr.grad, rtol=2e-4, atol=3e-4 * float(wr.grad.abs().max()))


def test_unet_bf16_vs_f32_end_to_end(ops_bf16):
    ops = ops_bf16
    from adm_amd.unet.uncond_unet import EDMPrecond
    cfg = unet_ref.default_cfg(variant="uncond_unet", model_channels=64, num_blocks=1, dropout=0.0)
    kw = {k: cfg[k] for k in ("model_channels", "channel_mult", "channel_mult_emb", "num_blocks", "attn_resolutions",
                              "dropout", "augment_dim")}
    m = EDMPrecond(img_resolution=32, img_channels=3, **kw)
    m.load_state_dict(fill.filled_state_dict(unet_ref.param_shapes(cfg)))
    m = m.cuda().eval()
    x = fill.hash_tensor((2, 3, 32, 32), "x", 1.0).cuda()
    sigma = torch.tensor([0.05, 0.7]).cuda()
    gx = fill.hash_tensor((2, 3, 32, 32), "gx", 1.0).cuda()

    def run():
        for p in m.parameters():
            p.grad = None
        dx, dy = m(x, sigma)
        ((dx * gx).sum() + (dy * gx).sum()).backward()
        g = torch.cat([p.grad.reshape(-1) for p in m.parameters() if p.grad is not None])
        return dx.detach(), dy.detach(), g

    a16 = run()
    ops.set_compute_precision("f32")
    a32 = run()
    for u, v in zip(a16[:2], a32[:2]):
        assert float((u - v).abs().max()) <= 3e-2 * float(v.abs().max())
        assert float((u - v).abs().max()) > 0          # the bf16 path really ran
    cos = float(torch.dot(a16[2].double(), a32[2].double()) / (a16[2].double().norm() * a32[2].double().norm()))
    assert cos >= 0.999, cos


@pytest.mark.parametrize("C,H,drop,with_ss", [(192, 32, 0.1, True), (384, 16, 0.0, False), (768, 8, 0.1, True), (64, 4, 0.0, True)])
def test_group_norm_bf16_storage_output(ops_bf16, C, H, drop, with_ss):
    """bf16-storage mode (BASELINE configs[2], 'bf16 activations'): adm_gn_fwd_bf16out must write exactly the round-to-nearest-even
    bf16 of what adm_gn_fwd writes in f32 -- multi-pass (32x32) and one-launch (<= 16x16) kernels, with scale/shift and dropout."""
    ops = ops_bf16
    B = 4
    x = fill.hash_tensor((B, H, H, C), f"gsx{C}{H}", 1.5).cuda()
    g, b = (1 + fill.hash_tensor((C,), "gsg", 0.2)).cuda(), fill.hash_tensor((C,), "gsb", 0.1).cuda()
    ss = fill.hash_tensor((B, 2 * C), "gss", 0.1).cuda() if with_ss else None
    y32 = ops.group_norm_act(x, g, b, ss, silu=True, drop_p=drop, seed=1234)
    carrier = ops.group_norm_act(x, g, b, ss, silu=True, drop_p=drop, seed=1234, to_conv=True)
    y16 = carrier._adm_bf16
    assert y16.dtype == torch.bfloat16 and y16.shape == x.shape
    assert torch.equal(y16, y32.to(torch.bfloat16))


def test_unet_bf16_storage_equals_rounding_on_load(ops_bf16, monkeypatch):
    """The storage mode changes WHERE the rounding happens, not what is computed: the forward outputs of the reduced UNet are
    bit-identical with ADM_BF16_STORAGE on (bf16 GroupNorm outputs read directly by the convs) and off (f32 outputs rounded in the
    conv loaders).  The parameter gradients agree at the bf16 level only: with stored bf16 activations the 3x3 / large 1x1 weight
    gradients run on the split-bf16 kernels, which keep dY EXACT (three-term split), while the direct bf16 kernel of the f32-storage
    mode rounds dY to bf16 on load."""
    ops = ops_bf16
    from adm_amd.unet.uncond_unet import EDMPrecond
    cfg = unet_ref.default_cfg(variant="uncond_unet", model_channels=64, num_blocks=1, dropout=0.0)
    kw = {k: cfg[k] for k in ("model_channels", "channel_mult", "channel_mult_emb", "num_blocks", "attn_resolutions",
                              "dropout", "augment_dim")}
    m = EDMPrecond(img_resolution=32, img_channels=3, **kw)
    m.load_state_dict(fill.filled_state_dict(unet_ref.param_shapes(cfg)))
    m = m.cuda().eval()
    x = fill.hash_tensor((2, 3, 32, 32), "x", 1.0).cuda()
    sigma = torch.tensor([0.05, 0.7]).cuda()
    gx = fill.hash_tensor((2, 3, 32, 32), "gx", 1.0).cuda()

    def run(storage):
        monkeypatch.setattr(ops, "BF16_STORAGE", storage)
        for p in m.parameters():
            p.grad = None
        dx, dy = m(x, sigma)
        ((dx * gx).sum() + (dy * gx).sum()).backward()
        return dx.detach(), dy.detach(), [p.grad.clone() for p in m.parameters() if p.grad is not None]

    on, off = run(True), run(False)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert len(on[2]) == len(off[2]) > 50
    for u, v in zip(on[2], off[2]):
        assert float((u - v).abs().max()) <= 1e-2 * max(float(v.abs().max()), 1e-3)


@pytest.mark.parametrize("B,cin,cout,H,up,ks", [(8, 64, 96, 32, False, 3), (4, 96, 64, 16, True, 3), (16, 192, 192, 16, False, 3),
                                                (8, 64, 128, 32, False, 1), (3, 96, 96, 8, False, 1)])
def test_wgrad_x6_bf16_activations_equal_f32_kernel_on_rounded_x(ops_bf16, B, cin, cout, H, up, ks):
    """adm_conv_wgrad_x6_bf16a / adm_gemm_wgrad_x6_bf16a (x stored as bf16) against the f32-input kernels fed the same values
    widened to f32: identical products, split-K atomics reorder the sums (1e-6 of the scale)."""
    from adm_amd import hip
    gpu = torch.device("cuda:0")
    Hin = H // 2 if up else H
    x = fill.hash_tensor((B, Hin, Hin, cin), f"xb{cin}{cout}{H}", 1.0)
    dy = fill.hash_tensor((B, H, H, cout), f"gb{cin}{cout}{H}", 0.05)
    x16 = x.to(torch.bfloat16).to(gpu)
    xf = x16.to(torch.float32)
    dyd = dy.to(gpu)
    planes = 12 if ks == 3 else 1
    out = []
    for which in (0, 1):
        dwp = torch.zeros((cout, planes * cin), device=gpu)
        db = torch.zeros((cout,), device=gpu)
        if ks == 3:
            if which:
                hip.call("adm_conv_wgrad_x6_bf16a", hip.ptr(x16), hip.ptr(dyd), hip.ptr(dwp), hip.ptr(db), B, H, H, cin, cin, cout, cout, 0,
                         int(up))
            else:
                hip.call("adm_conv_wgrad_x6_up" if up else "adm_conv_wgrad_x6", hip.ptr(xf), hip.ptr(dyd), hip.ptr(dwp), hip.ptr(db), B, H, H,
                         cin, cin, cout, cout, 0)
        else:
            hip.call("adm_gemm_wgrad_x6_bf16a" if which else "adm_gemm_wgrad_x6", hip.ptr(x16 if which else xf), hip.ptr(dyd), hip.ptr(dwp),
                     hip.ptr(db), B * H * H, cin, cin, cout, cout, 0)
        torch.cuda.synchronize()
        out.append((dwp.cpu(), db.cpu()))
    scale = float(out[0][0].abs().max())
    assert scale > 0
    assert float((out[0][0] - out[1][0]).abs().max()) <= 2e-6 * scale
    assert float((out[0][1] - out[1][1]).abs().max()) <= 2e-6 * float(out[0][1].abs().max())


# ------------------------------------------------------------------------------------------------ storage mode at full width
BAR_A = 1e-5        # tests/test_hip_accuracy.py: e_max against fp64 (fp64ref.errors), every path


def _f32_kernels(ops, mp, x, w, b, res, dy, ks):
    """The same conv on the f32-MFMA kernels (no split format, no Winograd-domain 16-bit images), forward and backward, on the values
    given: what bar B compares against."""
    mp.setattr(ops, "COMPUTE", "f32")
    mp.setattr(ops, "BF16X6", False)
    mp.setattr(ops, "FP16X3", False)
    xd, wd = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = ops.conv2d(xd, wd, b, res)
    y.backward(dy)
    ops.flush_deferred_unpack()
    torch.cuda.synchronize()
    mp.undo()
    return y.detach(), xd.grad, wd.grad


@pytest.mark.parametrize("B,H,cout,ks,wgrad", [(8, 16, 192, 3, "adm_conv_wgrad_x6_bf16a"), (4, 16, 576, 1, "adm_conv_wgrad_bf16a"),
                                               (4, 12, 192, 3, "adm_conv_wgrad_bf16a")],
                         ids=["3x3-16x16", "1x1-qkv-shaped", "3x3-12x12"])
def test_storage_mode_gn_into_conv_vs_fp64(ops_bf16, B, H, cout, ks, wgrad):
    """group_norm_act(to_conv=True) -> conv2d with a residual at 192 channels, forward and backward, in the storage mode: the conv reads
    the stored bf16 values (adm_conv_fwd_bf16a) and the weight gradient takes the split-bf16 Winograd kernel on a power-of-two map of
    >= 2048 pixels, the direct adm_conv_wgrad_bf16a below the split-GEMM threshold and on a 12x12 map.  Output and gradients against
    fp64 of the values AS STORED (and of the operands rounded as each kernel rounds them: the data gradient dy and w, the direct
    weight gradient dy, the split one nothing), on bars A and B."""
    ops = ops_bf16
    assert ops.bf16_storage()
    C = 192
    tag = f"st{B}{H}{cout}{ks}"
    x = fill.hash_tensor((B, H, H, C), tag + "x", 1.5).cuda().requires_grad_(True)
    gam, bet = (1 + fill.hash_tensor((C,), tag + "g", 0.2)).cuda(), fill.hash_tensor((C,), tag + "b", 0.1).cuda()
    w = fill.hash_tensor((cout, C, ks, ks), tag + "w", 1.0 / math.sqrt(C * ks * ks)).cuda()
    b = fill.hash_tensor((cout,), tag + "c", 0.5).cuda()
    res = fill.hash_tensor((B, H, H, cout), tag + "r", 1.0).cuda()
    dy = fill.hash_tensor((B, H, H, cout), tag + "d", 1.0).cuda()
    wd, bd, rd = w.clone().requires_grad_(True), b.clone().requires_grad_(True), res.clone().requires_grad_(True)
    names, grads = [], {}
    with pytest.MonkeyPatch.context() as mp:
        orig_call = ops.call
        mp.setattr(ops, "call", lambda name, *a: (names.append(name), orig_call(name, *a))[1])
        h = ops.group_norm_act(x, gam, bet, None, silu=True, to_conv=True)
        h16 = h._adm_bf16
        h.register_hook(lambda g: grads.__setitem__("dh", g.clone()))
        y = ops.conv2d(h, wd, bd, rd)
        y.backward(dy)
        ops.flush_deferred_unpack()
        torch.cuda.synchronize()
    assert "adm_gn_fwd_bf16out" in names and names.count("adm_conv_fwd_bf16a") == 1 and names.count("adm_conv_fwd_bf16") == 1, names
    assert wgrad in names and not any(n.startswith("adm_conv_wgrad") and n != wgrad for n in names), names
    assert torch.equal(rd.grad, dy) and bool(torch.isfinite(x.grad).all())
    hf = h16.to(torch.float32)
    dy_w = dy if wgrad == "adm_conv_wgrad_x6_bf16a" else r16(dy)          # the split kernel keeps dy exact (three-term split)
    ref = fp64ref.conv(hf, r16(w), b, res)
    ref_dx = fp64ref.conv(hf, r16(w), dy=r16(dy))["dx"]
    ref_dw = fp64ref.conv(hf, w, dy=dy_w)["dw"]
    ref_db = fp64ref.conv(hf, w, b, dy=dy)["db"]
    with pytest.MonkeyPatch.context() as mp:
        y32, dx32, _ = _f32_kernels(ops, mp, hf, r16(w), b, res, r16(dy), ks)
    with pytest.MonkeyPatch.context() as mp:
        dw32 = _f32_kernels(ops, mp, hf, w, b, res, dy_w, ks)[2]
    bad = []
    for out, got, rf, g32 in (("y", y.detach(), ref["y"], y32), ("dx", grads["dh"], ref_dx, dx32), ("dw", wd.grad, ref_dw, dw32),
                              ("db", bd.grad, ref_db, None)):
        e = fp64ref.errors(got, *rf)
        line = f"{tag} {out}: e_max {e[0]:.2e} e_rms {e[1]:.2e}"
        if e[0] > BAR_A:
            bad.append("bar A: " + line)
        if g32 is not None:
            e32 = fp64ref.errors(g32, *rf)
            ok, rm, rr = fp64ref.bar_b(e, e32)
            line += f"  f32 {e32[0]:.2e}/{e32[1]:.2e}  ratios {rm:.2f}/{rr:.2f}"
            if not ok:
                bad.append("bar B: " + line)
        print(line)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("row", [r for r in gn_cases.GRID if r[2] % 64 == 0], ids=gn_cases.row_id)
def test_group_norm_bf16_storage_output_over_the_plan_grid(ops_bf16, row):
    """adm_gn_fwd_bf16out on every launch plan of the GroupNorm grid it can take (C % 64 == 0), with scale/shift, SiLU and dropout: the
    stored values are the round-to-nearest-even bf16 of what adm_gn_fwd writes in f32 on the same plan."""
    ops = ops_bf16
    H, W, C, _, eps, B, _ = row
    c = gn_cases.make_case(row, "plain")
    x, g, b, ss = (c[k].cuda() for k in ("x", "gamma", "beta", "ss"))
    kw = dict(silu=True, drop_p=0.1, seed=4321, groups=gn_cases.groups_of(row), eps=eps)
    y32 = ops.group_norm_act(x, g, b, ss, **kw)
    y16 = ops.group_norm_act(x, g, b, ss, to_conv=True, **kw)._adm_bf16
    assert y16.dtype == torch.bfloat16 and y16.shape == x.shape
    assert bool((y32 == 0).any()) and bool((y32 != 0).any())                      # the dropout really dropped
    assert torch.equal(y16, y32.to(torch.bfloat16))


@pytest.mark.parametrize("storage", [False, True], ids=["f32-storage", "bf16-storage"])
def test_weight_change_in_place_reaches_the_bf16_operands(ops_bf16, monkeypatch, storage):
    """The bf16 weight copies (fwd16 / bwd16) are rebuilt from the f32 operands, which repack_all() refreshes only if they were read:
    after an in-place change of the weight as the optimiser makes it (through the storage, no version bump) and repack_all(), forward
    and backward equal, bit for bit, a fresh layer built from the new values -- also when the step before the change ran no backward
    (the data-gradient operand then goes stale and is refreshed on its next read)."""
    ops = ops_bf16
    monkeypatch.setattr(ops, "BF16_STORAGE", storage)
    B, H, C, co = 2, 8, 64, 128
    xv = fill.hash_tensor((B, H, H, C), "wrx", 1.0).cuda()
    gam, bet = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    dy = fill.hash_tensor((B, H, H, co), "wrd", 1.0).cuda()
    w0 = fill.hash_tensor((co, C, 3, 3), "wrw", 1.0 / 24).cuda()
    delta = fill.hash_tensor((co, C, 3, 3), "wru", 0.01).cuda()
    bias = fill.hash_tensor((co,), "wrb", 0.5).cuda()

    def step(weight, backward=True):
        x = xv.clone().requires_grad_(True)
        weight.grad = None
        h = ops.group_norm_act(x, gam, bet, None, silu=True, to_conv=True)
        assert (getattr(h, "_adm_bf16", None) is not None) == storage
        y = ops.conv2d(h, weight, bias)
        if backward:
            y.backward(dy)
            ops.flush_deferred_unpack()
        torch.cuda.synchronize()
        return (y.detach().clone(),) + ((x.grad.clone(), weight.grad.clone()) if backward else ())

    layer = torch.nn.Parameter(w0.clone())
    first = step(layer)
    for backward_before in (True, False):
        if not backward_before:                         # an optimiser step whose successor runs no backward: only the forward
            ops.repack_all()                            # operand is read between the two repacks
            step(layer, backward=False)
        version = layer._version
        layer.data.add_(delta)                          # as the fused optimiser: the values change, the version does not
        assert layer._version == version
        ops.repack_all()
        ent = layer._adm_packed
        assert ent.fwd16 is None and ent.bwd16 is None
        assert bool(ent._stale & 2) == (not backward_before)      # the data-gradient operand was left out of the repack
        got = step(layer)
        assert layer._adm_packed is ent                 # the same entry, refreshed -- not a rebuild
        fresh = step(torch.nn.Parameter(layer.detach().clone()))
        for u, v in zip(got, fresh):
            assert torch.equal(u, v)
        assert not torch.equal(got[0], first[0])
