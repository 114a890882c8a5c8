"""CPU: the fp64 reference of tests/fp64ref.py against torch's own fp64 operators, and the accuracy bars of
tests/test_hip_accuracy.py on emulated precision defects of the split formats (no GPU needed)."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import fill

import fp64ref
import gn_cases
from parity import close
from test_hip_accuracy import BAR_A

_f64 = torch.float64


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("B,ci,co,H,W,ks,up,stride,pad", [
    (2, 5, 7, 6, 5, 3, False, 1, None),        # ragged channels and an odd, non-square map
    (1, 3, 4, 4, 6, 3, True, 1, None),         # fused nearest x2
    (3, 6, 5, 7, 7, 1, False, 1, None),        # 1x1
    (2, 4, 3, 9, 8, 3, False, 2, (0, 1)),      # the autoencoder's Downsample: pad (0, 1), stride 2
    (1, 3, 5, 11, 10, 7, False, 1, (3, 3)),    # a 7x7 stem
    (2, 4, 6, 8, 9, 4, False, 2, (1, 1)),      # a 4x4 stride-2 down-sampling conv
])
def test_conv_reference_matches_torch_fp64(B, ci, co, H, W, ks, up, stride, pad):
    """Forward, data, weight and bias gradients, with a bias and a residual, to 1e-12 of F.conv2d / conv_transpose2d /
    conv2d_weight in fp64; mag equals the same operators on |operands|."""
    x = fill.hash_tensor((B, ci, H, W), "r.x", 1.0, _f64)
    w = fill.hash_tensor((co, ci, ks, ks), "r.w", 1.0, _f64)
    b = fill.hash_tensor((co,), "r.b", 1.0, _f64)
    lo, hi = (ks // 2, ks // 2) if pad is None else pad
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x

    def tconv(xx, ww):
        return F.conv2d(F.pad(xx, (lo, hi, lo, hi)), ww, stride=stride)

    Ho = tconv(xin, w).shape[2]
    Wo = tconv(xin, w).shape[3]
    res = fill.hash_tensor((B, co, Ho, Wo), "r.res", 1.0, _f64)
    dy = fill.hash_tensor((B, co, Ho, Wo), "r.dy", 1.0, _f64)
    got = fp64ref.conv(_nhwc(x), w, b, _nhwc(res), _nhwc(dy), up=up, stride=stride, pad=pad)
    for part, f in (("ref", lambda t: t), ("mag", lambda t: t.abs())):
        xr, wr = f(x).detach().requires_grad_(True), f(w).detach().requires_grad_(True)
        xi = F.interpolate(xr, scale_factor=2, mode="nearest") if up else xr
        y = tconv(xi, wr) + f(b).view(1, co, 1, 1) + f(res)
        y.backward(f(dy))
        want = {"y": y.detach(), "dx": xr.grad, "dw": wr.grad, "db": f(dy).sum(dim=(0, 2, 3))}
        i = 0 if part == "ref" else 1
        for n, t in want.items():
            g = got[n][i]
            g = _nchw(g) if g.dim() == 4 and n in ("y", "dx") else g
            assert g.shape == t.shape, (n, g.shape, t.shape)
            assert float((g - t).abs().max()) <= 1e-12 * max(1.0, float(t.abs().max())), (part, n)
    if stride == 1 and not up and pad is None:      # the plain conv's gradients are torch's named operators
        assert torch.allclose(_nchw(got["dx"][0]), F.conv_transpose2d(dy, w, padding=ks // 2), rtol=0, atol=1e-12)
        assert torch.allclose(got["dw"][0], torch.nn.grad.conv2d_weight(x, w.shape, dy, padding=ks // 2), rtol=0, atol=1e-12)


def test_linear_weight_reference():
    """A [Co, Ci] Linear weight is a 1x1 conv over [B, 1, 1, Ci]."""
    x = fill.hash_tensor((3, 1, 1, 10), "l.x", 1.0, _f64)
    w = fill.hash_tensor((4, 10), "l.w", 1.0, _f64)
    got = fp64ref.conv(x, w)
    assert torch.allclose(got["y"][0].reshape(3, 4), x.reshape(3, 10) @ w.t(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("heads,L", [(1, 16), (3, 64)])
def test_attention_reference_matches_autograd(heads, L):
    """Forward and backward against torch autograd in fp64, in the kernels' layout ((q | k | v) x 64 channels per head)."""
    B = 2
    qkv = fill.hash_tensor((B, L, heads * 192), "a.qkv", 2.0, _f64)
    dout = fill.hash_tensor((B, L, heads * 64), "a.do", 1.0, _f64)
    got = fp64ref.attention(qkv, heads, dout)
    q = qkv.clone().requires_grad_(True)
    t = q.reshape(B, L, heads, 3, 64)
    qq, kk, vv = (t[:, :, :, i].transpose(1, 2) for i in range(3))
    o = torch.softmax(qq @ kk.transpose(-1, -2) / math.sqrt(64), dim=-1) @ vv
    o = o.transpose(1, 2).reshape(B, L, heads * 64)
    o.backward(dout)
    assert float((got["out"][0] - o.detach()).abs().max()) <= 1e-12
    assert float((got["dqkv"][0] - q.grad).abs().max()) <= 1e-12
    # mag bounds |ref| elementwise (it is the same sums over |terms|)
    assert bool((got["out"][1] >= got["out"][0].abs() - 1e-12).all())
    assert bool((got["dqkv"][1] >= got["dqkv"][0].abs() - 1e-12).all())


@pytest.mark.parametrize("row", [gn_cases.GRID[i] for i in (5, 6, 12)], ids=gn_cases.row_id)
def test_group_norm_reference_matches_autograd(row):
    """fp64ref.group_norm (written from the definition) against torch.autograd on F.group_norm(double) with the same scale/shift,
    SiLU, mask and residual gradient, to 1e-12; without scale/shift and SiLU too; every mag bounds |ref|."""
    H, W, C, _, eps, B, _ = row
    G = gn_cases.groups_of(row)
    c = {k: v.double() for k, v in gn_cases.make_case(row, "plain").items()}
    keep = (fill.hash_tensor((B, H, W, C), "gn.keep", 1.0, _f64) > -0.8).double() / 0.9
    for silu, ss, kp, add in ((True, c["ss"], keep, c["addend"]), (False, None, None, None), (True, c["ss"][:1], None, None)):
        got = fp64ref.group_norm(c["x"], c["gamma"], c["beta"], ss, groups=G, eps=eps, silu=silu, keep=kp, addend=add, dy=c["dy"])
        want = gn_cases.torch_composition(c["x"], c["gamma"], c["beta"], ss, groups=G, eps=eps, silu=silu, keep=kp, addend=add,
                                          dy=c["dy"])
        assert set(got) == set(want)
        for n, t in want.items():
            ref, mag = got[n]
            assert ref.shape == t.shape and mag.shape == t.shape, (n, ref.shape, mag.shape, t.shape)
            assert float((ref - t).abs().max()) <= 1e-12 * max(1.0, float(t.abs().max())), (n, silu)
            assert bool((mag >= ref.abs() * (1 - 1e-12)).all()), n
    y_only = fp64ref.group_norm(c["x"], c["gamma"], c["beta"], None, groups=G, eps=eps, silu=True)
    assert set(y_only) == {"y"}


@pytest.mark.parametrize("row", gn_cases.GRID, ids=gn_cases.row_id)
def test_group_norm_bar_leaves_room_for_fp32(row):
    """The bar of tests/test_hip_groupnorm.py (BAR_A on every output) against what plain fp32 arithmetic does: the fp32 torch
    composition on the CPU stays below a quarter of it at every grid shape and data kind (errors printed)."""
    H, W, C, _, eps, B, _ = row
    G = gn_cases.groups_of(row)
    for kind in gn_cases.KINDS:
        c = gn_cases.make_case(row, kind)
        kw = dict(groups=G, eps=eps, silu=True, addend=c["addend"], dy=c["dy"])
        ref = fp64ref.group_norm(c["x"], c["gamma"], c["beta"], c["ss"], **kw)
        got = gn_cases.torch_composition(c["x"], c["gamma"], c["beta"], c["ss"], **kw)
        e = {n: fp64ref.errors(got[n], *ref[n])[0] for n in ref}
        print(f"{gn_cases.row_id(row)} {kind}: " + " ".join(f"{n} {v:.2e}" for n, v in e.items()))
        for n, v in e.items():
            assert v <= BAR_A / 4, (kind, n, v)


def test_errors_are_relative_to_mag():
    ref = torch.tensor([1.0, -2.0, 0.0], dtype=_f64)
    mag = torch.tensor([2.0, 4.0, 0.0], dtype=_f64)
    got = torch.tensor([1.5, -2.0, 0.0])
    e_max, e_rms = fp64ref.errors(got, ref, mag)
    assert e_max == pytest.approx(0.5 / 4.0)
    assert e_rms == pytest.approx(math.sqrt(0.25 / 3) / math.sqrt(20.0 / 3))


# ------------------------------------------------------------------------------------------------ the bars have teeth
def _h3_drop_low_term(t, bound):
    """The fp16 split of the kernels with its LOW term dropped: s a -> fp16(s a) / s, s = the power of two with s * bound <= 16000
    (split_scale of csrc/split_format.h)."""
    s = 2.0 ** math.floor(math.log2(16000.0 / bound))
    return (t * s).to(torch.float16).to(_f64) / s


def _bf16_three_terms(t):
    a0 = t.to(torch.bfloat16).to(torch.float32)
    a1 = (t - a0).to(torch.bfloat16).to(torch.float32)
    a2 = (t - a0 - a1).to(torch.bfloat16).to(torch.float32)
    return a0, a1, a2


def _cifar_like():
    B, C, H = 2, 192, 16
    x = fill.hash_tensor((B, C, H, H), "bar.x", 1.0)
    w = fill.hash_tensor((C, C, 3, 3), "bar.w", 1.0 / math.sqrt(C * 9))
    ref = fp64ref.conv(_nhwc(x), w)["y"]
    e32 = fp64ref.errors(_nhwc(F.conv2d(x, w, padding=1)), *ref)       # torch's fp32 CPU conv: the f32 kernel's stand-in
    return x, w, ref, e32


def test_bar_b_rejects_a_dropped_fp16_low_term():
    """The bug class of the fp16 split format: one operand (the activations) keeps only its high fp16 term (relative error up to
    2^-12).  Bar B rejects it by at least 5x against torch's fp32 conv.  parity.close sits at the edge of it: here a handful of
    elements exceed its 1e-4 absolute term (printed), on other data it passes -- it cannot be relied on to see the defect."""
    x, w, ref, e32 = _cifar_like()
    xd = _h3_drop_low_term(x.double(), float(x.abs().max()))
    y = fp64ref.conv(_nhwc(xd), w)["y"][0]
    e = fp64ref.errors(y, *ref)
    ok, r_max, r_rms = fp64ref.bar_b(e, e32)
    print(f"fp16 low term dropped: e_max {e[0]:.3e} e_rms {e[1]:.3e}; fp32 conv e_max {e32[0]:.3e} e_rms {e32[1]:.3e}; "
          f"bar B ratios (error / limit): e_max {r_max:.1f}x, e_rms {r_rms:.1f}x")
    try:                                               # the existing op-level bar: reported, not asserted (see below)
        close(_nchw(y), _nchw(ref[0]))
        verdict = "accepts"
    except AssertionError:
        verdict = "rejects"
    d = (_nchw(y) - _nchw(ref[0])).abs()
    print(f"parity.close {verdict} it: max |err| / max |ref| = {float(d.max()) / float(ref[0].abs().max()):.2e} (its atol: 1e-4)")
    assert not ok and max(r_max, r_rms) >= 5.0, (r_max, r_rms)


def test_bar_b_on_a_dropped_third_bf16_term():
    """The six-bf16-product format with the third bf16 term of the activations dropped (relative error ~2^-17): smaller than the
    fp16 defect.  The margin is printed as measured."""
    x, w, ref, e32 = _cifar_like()
    a0, a1, _ = _bf16_three_terms(x)
    y = fp64ref.conv(_nhwc(a0.double() + a1.double()), w)["y"][0]
    e = fp64ref.errors(y, *ref)
    ok, r_max, r_rms = fp64ref.bar_b(e, e32)
    print(f"third bf16 term dropped: e_max {e[0]:.3e} e_rms {e[1]:.3e}; fp32 conv e_max {e32[0]:.3e} e_rms {e32[1]:.3e}; "
          f"bar B ratios: e_max {r_max:.2f}x, e_rms {r_rms:.2f}x")
    close(_nchw(y), _nchw(ref[0]))
    assert not ok, (r_max, r_rms)


def test_exact_splits_pass_bar_b():
    """Control: the full three-term bf16 split (exact) and the two-term fp16 split computed in fp64 are inside bar B."""
    x, w, ref, e32 = _cifar_like()
    a0, a1, a2 = _bf16_three_terms(x)
    y = fp64ref.conv(_nhwc(a0.double() + a1.double() + a2.double()), w)["y"][0]
    assert fp64ref.bar_b(fp64ref.errors(y, *ref), e32)[0]
