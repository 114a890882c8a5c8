"""GPU: the fp16 split format where its bounds can fail.

Every fp16-format kernel scales an f32 operand by a power of two taken from a BOUND (a device vector >= max |operand|) and stores the
scaled value as two fp16 terms (split_scale, csrc/split_format.h: s * bound <= 16000, so that the Winograd transforms' sums of four stay
below 65504).  These tests put operands at the edge of that claim (worst-case sign patterns at an exact bound, bounds where the
scale changes exponent, zeros, magnitudes far from 1) against fp64, and check the bookkeeping that carries the bounds: a gradient
summed in place after its bound was registered, every consumer under ADM_AMAX_CHECK semantics on each model family, weights that do
not fit the fixed weight scale, and the pool the bound vectors come from when three streams share it."""
import ctypes
import itertools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import fill

from parity import close  # noqa: E402  (tests/parity.py: the north_star tolerance, elementwise)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _amax(t):
    from adm_amd import ops as _ops
    return _ops.amax_vector(t)


def _kinds(ops):
    return [k[0] for k in ops.PROFILE]


def _worst(shape, a):
    """a * (-1)^(floor(i/2) + floor(j/2)) (+ the same shifted by one pixel in the odd batch items): on every 4x4 input tile of
    F(2x2,3x3) the corners carry +,-,-,+ (B^T d B reaches 4a), and on every patch of the weight gradient's F(3x3,2x2) both the X side
    ((r0 - r2)(c0 - c2)) and the dY side ((r0 + r1)(c0 + c1)) reach 4a as well."""
    B, C, H, W = shape
    i, j = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    out = torch.empty(shape)
    for b in range(B):
        o = b & 1
        out[b] = (1.0 - 2.0 * (((i + o) // 2 + (j + o) // 2) % 2).float()) * a
    return out


# operand cases: (name, bound of x, bound of dy, x generator) -- the bound is always EXACT (loose = 1)
_BELOW = lambda v: float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(0.0)))
_ABOVE = lambda v: float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(1e30)))
CASES = [
    ("worst-1", 1.0, 1.0),
    ("pow2", 2.0, 0.5),                                  # exact powers of two
    ("below-pow2", _BELOW(2.0), _BELOW(0.5)),           # just below a power of two
    ("s-max", 15.625, 15.625),                           # 16000 / 2^10: s * bound = 16000 exactly (the largest scaled value the rule allows)
    ("s-max-below", _BELOW(15.625), _BELOW(15.625)),
    ("s-max-above", _ABOVE(15.625), _ABOVE(0.48828125)),  # ... and where frexpf steps to the next exponent
    ("tiny", 1e-6, 1e-6),                               # the model's ends: gradients of 1e-6
    ("huge", 1e4, 1e4),
    ("zeros", 0.0, 0.0),                                # all zeros, bound 0 (behind the zero-initialised output convs at step 0)
]


def _rel_err(got, ref, scale):
    return float((got.double() - ref).abs().max()) / max(scale, 1e-300)


# ------------------------------------------------------------------------------------------------ A: operands at the edge, vs fp64
@pytest.mark.parametrize("name,ax,ag", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("ks", [3, 1])
def test_conv_h3_operands_at_the_edge_vs_fp64(ops, monkeypatch, name, ax, ag, ks):
    """3x3 (adm_conv_fwd_wino2d_h3 forward and data gradient, adm_conv_wgrad_x6_h3) and 1x1 (adm_gemm_x6_h3 forward and data gradient,
    adm_gemm_wgrad_x6_h3) on operands whose every element sits at the exact bound with the sign pattern that drives the Winograd
    transforms to 4x the bound: finite, within the parity bar of an fp64 convolution, and at the f32-MFMA kernel's error against
    fp64 (relative to max sum |a b|).  The launch record proves the fp16-format kernels ran."""
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    monkeypatch.setattr(ops, "GEMM_X6_MIN_M", 1)
    B, cin, cout, H = 2, 128, 128, 16
    x = _worst((B, cin, H, H), ax)
    gy = _worst((B, cout, H, H), ag)
    if name == "worst-1":      # the same pattern with hashed magnitudes inside the bound (the bound stays exact: the largest element is kept)
        x = x * (0.5 + 0.5 * fill.hash_tensor(x.shape, "bx", 1.0).abs()); x[0, 0, 0, 0] = ax
        gy = gy * (0.5 + 0.5 * fill.hash_tensor(gy.shape, "bg", 1.0).abs()); gy[1, 0, 1, 1] = ag
    w = fill.hash_tensor((cout, cin, ks, ks), f"bw{ks}", 1.0 / math.sqrt(cin * ks * ks))
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y_ref = F.conv2d(xr, wr, padding=ks // 2)
    (y_ref * gy.double()).sum().backward()
    s_y = float(F.conv2d(x.double().abs(), w.double().abs(), padding=ks // 2).max())
    s_dx = float(F.conv_transpose2d(gy.double().abs(), w.double().abs(), padding=ks // 2).max())
    s_dw = float(F.conv2d(x.double().abs().transpose(0, 1), gy.double().abs().transpose(0, 1), padding=ks // 2).max())
    errs = {}
    for mode in ("f32", "h3"):
        monkeypatch.setattr(ops, "BF16X6", mode == "h3")
        monkeypatch.setattr(ops, "_get_amax", (lambda t: _amax(t)) if mode == "h3" else (lambda t: None))     # dy's bound: exact
        xd = nhwc(x).requires_grad_(True)
        wd = dev(w).requires_grad_(True)
        monkeypatch.setattr(ops, "PROFILE", [])
        y = ops.conv2d(xd, wd, None, amax=_amax(xd) if mode == "h3" else None)
        fwd = _kinds(ops)
        monkeypatch.setattr(ops, "PROFILE", [])
        (y * nhwc(gy)).sum().backward()
        bwd = _kinds(ops)
        monkeypatch.setattr(ops, "PROFILE", None)
        if mode == "h3":
            k = "wino2h3" if ks == 3 else "gemmh3"
            assert fwd == [k], fwd
            assert bwd.count(k) == 1 and bwd.count("wgrad_wino2h3" if ks == 3 else "wgrad_gemmh3") == 1, bwd
        for t in (y, xd.grad, wd.grad):
            assert bool(torch.isfinite(t).all()), (name, mode)
        yn, dxn = nchw(y)[:, :cout], nchw(xd.grad)[:, :cin]
        close(yn, y_ref.detach(), scale=s_y)
        close(dxn, xr.grad, scale=s_dx)
        close(wd.grad, wr.grad, scale=s_dw)
        errs[mode] = (_rel_err(yn, y_ref.detach(), s_y), _rel_err(dxn, xr.grad, s_dx), _rel_err(wd.grad.cpu(), wr.grad, s_dw))
    print(f"{name} ks={ks}: error / max sum|ab| (y, dx, dW): f32 MFMA {errs['f32']}, fp16 format {errs['h3']}")
    for i in range(3):
        assert errs["h3"][i] <= max(2.0 * errs["f32"][i], 4e-7), (name, i, errs)


@pytest.mark.parametrize("L", [64, 1024])
@pytest.mark.parametrize("aq,ag", [(1.0, 1.0), (15.625, 15.625), (_BELOW(15.625), 1e-6), (1e-3, 1e3)])
def test_attention_h3_at_the_bound_vs_fp64(ops, monkeypatch, L, aq, ag):
    """The attention forward and backward on the fp16 format with every row of V at the bound of qkv (alternating +aq / -aq by key)
    and dout = ag everywhere, so that dP = dO V^T reaches 64 aq ag and the dS bound 128 aq ag of attention_h3.hip is the live limit:
    one 256-key chunk (L = 64) and the chunked online softmax (L = 1024), exact bounds, finite and at the f32 kernel's error vs fp64."""
    B, heads = 2, 1
    h = int(math.isqrt(L))
    C = 64 * heads
    q = fill.hash_tensor((B, 64, L), f"baq{L}", 0.05 * aq)
    k = fill.hash_tensor((B, 64, L), f"bak{L}", 0.05 * aq)
    v = (1.0 - 2.0 * (torch.arange(L) % 2).float()).view(1, 1, L).expand(B, 64, L) * aq
    qkv = torch.stack([q, k, v], dim=2).reshape(B, 192, h, h)          # the oracle's channel order: [64 channels][q, k, v]
    packed = torch.stack([q, k, v], dim=1).reshape(B, 192, h, h)       # the kernels' order: [q, k, v][64 channels]
    from_packed = lambda t: t.reshape(B, 3, 64, h, h).transpose(1, 2).reshape(B, 192, h, h)
    gy = torch.full((B, C, h, h), ag)
    q64 = qkv.double().clone().requires_grad_(True)
    qq = q64.reshape(B, 64, 3, L)
    w64 = torch.softmax(torch.einsum("ncq,nck->nqk", qq[:, :, 0], qq[:, :, 1] / 8.0), dim=2)
    a64 = torch.einsum("nqk,nck->ncq", w64, qq[:, :, 2]).reshape(B, C, h, h)
    (a64 * gy.double()).sum().backward()
    errs = {}
    for mode in ("f32", "h3"):
        monkeypatch.setattr(ops, "ATTN_H3", mode == "h3")
        qd = nhwc(packed).requires_grad_(True)
        qd._adm_amax = _amax(qd)
        monkeypatch.setattr(ops, "_get_amax", (lambda t: _amax(t)) if mode == "h3" else (lambda t: None))
        monkeypatch.setattr(ops, "PROFILE", [])
        a = ops.attention(qd, heads)
        (a * nhwc(gy)).sum().backward()
        kinds = _kinds(ops)
        monkeypatch.setattr(ops, "PROFILE", None)
        assert kinds == (["attnh3", "attnh3"] if mode == "h3" else ["attn", "attn"]), kinds
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(qd.grad).all()), mode
        an, gn = nchw(a), from_packed(nchw(qd.grad))
        close(an, a64.detach())
        close(gn, q64.grad)
        errs[mode] = (_rel_err(an, a64.detach(), float(a64.abs().max())), _rel_err(gn, q64.grad, float(q64.grad.abs().max())))
    print(f"L={L} aq={aq} ag={ag}: error / max (out, dqkv): f32 {errs['f32']}, fp16 format {errs['h3']}")
    assert errs["h3"][0] <= max(3.0 * errs["f32"][0], 5e-7), errs
    assert errs["h3"][1] <= max(3.0 * errs["f32"][1], 1e-6), errs


# ------------------------------------------------------------------------------------------------ B.1: a gradient summed in place
@pytest.mark.parametrize("check", [False, True])
def test_gradient_summed_in_place_does_not_keep_the_first_addends_bound(ops, monkeypatch, check):
    """h = conv3x3(x) feeds two group_norm_act(..., to_conv=True) branches WITHOUT ops.fanout: autograd sums the two GroupNorm data
    gradients IN PLACE into the first one's buffer, whose registered bound is that addend's maximum.  The branches are identical and
    their upstream gradient is the worst-case sign pattern, so the sum is twice either addend and its Winograd transform reaches 4x
    the sum: with the stale bound the conv's data gradient overflows fp16.  The sum must be found unbound (or bound correctly): dx and
    dW match fp64, also under AMAX_CHECK."""
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    monkeypatch.setattr(ops, "AMAX_CHECK", check)
    B, C, H = 2, 64, 16
    x = torch.zeros(B, C, H, H)
    i, j = torch.arange(H).view(H, 1), torch.arange(H).view(1, H)
    x[:] = (1.0 - 2.0 * ((i + j) % 2).float())        # checkerboard: zero mean per group, orthogonal to the gradient's pattern
    x = x * (1.0 + 0.25 * torch.arange(C).float().view(1, C, 1, 1) / C)
    w0 = torch.zeros(C, C, 3, 3)
    w0[:, :, 1, 1] = torch.eye(C)                       # h = x (exactly)
    w0 += fill.hash_tensor(w0.shape, "ipw0", 1e-3)
    w1 = torch.zeros(C, C, 3, 3)
    w1[:, :, 1, 1] = torch.eye(C)
    gamma, beta = torch.ones(C), torch.zeros(C)
    gy = _worst((B, C, H, H), 15.0)                     # 15: s * 15 = 15360, close to the 16000 the scale allows
    # fp64 reference
    xr, w0r = x.double().requires_grad_(True), w0.double().requires_grad_(True)
    hr = F.conv2d(xr, w0r, padding=1)
    G = min(32, C // 4)
    loss = 0
    for _ in range(2):
        loss = loss + (F.conv2d(F.group_norm(hr, G, eps=1e-5), w1.double(), padding=1) * gy.double()).sum()
    loss.backward()
    # HIP
    reg, seen = [], []
    orig_reg = ops._reg_amax
    monkeypatch.setattr(ops, "_reg_amax", lambda t, slot: (reg.append(t.data_ptr()) if slot is not None else None, orig_reg(t, slot))[1])
    xd = nhwc(x).requires_grad_(True)
    w0d, w1d = dev(w0).requires_grad_(True), dev(w1)
    h = ops.conv2d(xd, w0d, None)
    h.register_hook(lambda g: seen.append(g.data_ptr()))
    out = 0
    for _ in range(2):
        out = out + (ops.conv2d(ops.group_norm_act(h, dev(gamma), dev(beta), None, silu=False, to_conv=True), w1d, None) * nhwc(gy)).sum()
    monkeypatch.setattr(ops, "PROFILE", [])
    out.backward()
    tags = [r[4] for r in ops.PROFILE]
    monkeypatch.setattr(ops, "PROFILE", None)
    assert seen and seen[0] in reg, "autograd did not sum the two gradients in place into a registered addend: the test proves nothing"
    assert any(t.startswith("dgrad-wino2") for t in tags), tags
    assert bool(torch.isfinite(xd.grad).all()) and bool(torch.isfinite(w0d.grad).all())
    close(nchw(xd.grad), xr.grad)
    close(w0d.grad, w0r.grad)


# ------------------------------------------------------------------------------------------------ B.2: every consumer checks its bound
def _h3_kinds(ops):
    return {k for k in _kinds(ops) if k.endswith("h3")}


def test_amax_check_uncond_unet_full_width(ops, monkeypatch):
    """The two-decoder uncond UNet at full width (B = 2) forward + backward with AMAX_CHECK: every bound a consumer reads (conv
    inputs, gradients by address, attention forward / backward, the weight gradients' x and dy) is verified against its tensor."""
    from test_hip_model import build_unet, small_inputs
    monkeypatch.setattr(ops, "AMAX_CHECK", True)
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)          # every 3x3 / 1x1 layer on the split kernels (the attention levels' too)
    monkeypatch.setattr(ops, "GEMM_X6_MIN_M", 1)
    gpu = torch.device("cuda:0")
    m, cfg, _ = build_unet("uncond_unet", gpu, full=True)
    m.train()
    x, sigma, aug = small_inputs(cfg)
    monkeypatch.setattr(ops, "PROFILE", [])
    dx, dy = m(x.to(gpu), sigma.to(gpu), augment_labels=aug.to(gpu))
    ((dx * fill.hash_tensor(dx.shape, "gx", 1.0).to(gpu)).sum() + (dy * fill.hash_tensor(dy.shape, "gy", 1.0).to(gpu)).sum()).backward()
    kinds = _h3_kinds(ops)
    monkeypatch.setattr(ops, "PROFILE", None)
    assert {"wino2h3", "wgrad_wino2h3", "gemmh3", "wgrad_gemmh3", "attnh3"} <= kinds, kinds
    assert bool(torch.isfinite(dx).all()) and all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)


def test_amax_check_latent_unet(ops, monkeypatch):
    """uncond_unet_sd_2 (single decoder, the latent configs' UNet) forward + backward with AMAX_CHECK (every 3x3 / 1x1 layer forced
    onto the split kernels)."""
    from oracle import unet_ref
    from test_hip_model import build_unet
    monkeypatch.setattr(ops, "AMAX_CHECK", True)
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    monkeypatch.setattr(ops, "GEMM_X6_MIN_M", 1)
    gpu = torch.device("cuda:0")
    m, cfg, _ = build_unet("uncond_unet_sd_2", gpu)
    m.train()
    B = 4
    x = fill.hash_tensor((B, 3, 32, 32), "lx", 1.0).to(gpu)
    sigma = torch.tensor([0.05, 0.7, 0.31, 0.999], device=gpu)
    monkeypatch.setattr(ops, "PROFILE", [])
    out = m(x, sigma)
    outs = out if isinstance(out, tuple) else (out,)
    sum((o * fill.hash_tensor(o.shape, f"lg{i}", 1.0).to(gpu)).sum() for i, o in enumerate(outs)).backward()
    kinds = _h3_kinds(ops)
    monkeypatch.setattr(ops, "PROFILE", None)
    assert {"wino2h3", "wgrad_wino2h3"} <= kinds, kinds
    assert all(bool(torch.isfinite(o).all()) for o in outs)


def test_amax_check_cond_unet(ops, monkeypatch):
    """cond_unet_sd (the conditional UNet) forward + backward with AMAX_CHECK, split kernels forced, against the run with the fp16
    format switched off.  (Its GroupNorms hand no bound to their convs, so none of its layers takes the fp16 format today: the
    launch record says which kernels ran.)"""
    from oracle import cond_unet_ref as R
    from test_hip_cond import build
    monkeypatch.setattr(ops, "AMAX_CHECK", True)
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    monkeypatch.setattr(ops, "GEMM_X6_MIN_M", 1)
    x = fill.hash_tensor((2, 3, 32, 32), "cond.x", 1.0).cuda()
    tt = torch.tensor([0.3, 0.85]).cuda()
    hm = [h.cuda() for h in R.cond_features(2, 32, 32)]
    res = {}
    for h3 in (True, False):
        monkeypatch.setattr(ops, "FP16X3", h3)
        m, cfg, _ = build()
        m.train()
        monkeypatch.setattr(ops, "PROFILE", [])
        y1, y2 = m(x, tt, hm)
        ((y1 * fill.hash_tensor(y1.shape, "cg1", 1.0).cuda()).sum() + (y2 * fill.hash_tensor(y2.shape, "cg2", 1.0).cuda()).sum()).backward()
        print("cond_unet_sd kernels:", sorted(set(_kinds(ops))))
        monkeypatch.setattr(ops, "PROFILE", None)
        assert bool(torch.isfinite(y1).all()) and bool(torch.isfinite(y2).all())
        res[h3] = (y1.detach(), y2.detach(), [p.grad.clone() for p in m.parameters() if p.grad is not None])
    close(res[True][0], res[False][0], rtol=1e-4, atol=1e-5); close(res[True][1], res[False][1], rtol=1e-4, atol=1e-5)
    for a, b in zip(res[True][2], res[False][2]):
        close(a, b, rtol=1e-3, atol=1e-4)


def test_amax_check_autoencoder_decode(ops, monkeypatch):
    """The KL autoencoder's decode with AMAX_CHECK, split kernels forced, against the decode with the fp16 format switched off.  (Only
    its input layout kernel writes a bound, and the 1x1 post-quant conv behind it is too narrow for the split kernels: the launch
    record says which kernels ran.)"""
    from test_hip_latent import build_ae
    monkeypatch.setattr(ops, "AMAX_CHECK", True)
    monkeypatch.setattr(ops, "WINO_MIN_M", 1)
    monkeypatch.setattr(ops, "GEMM_X6_MIN_M", 1)
    gpu = torch.device("cuda:0")
    ae, _, _ = build_ae(gpu, 32, (64, 64))
    z = fill.hash_tensor((2, 3, 16, 16), "aez", 2.0).to(gpu)
    res = {}
    for h3 in (True, False):
        monkeypatch.setattr(ops, "FP16X3", h3)
        monkeypatch.setattr(ops, "PROFILE", [])
        with torch.no_grad():
            res[h3] = ae.decode(z)
        print("autoencoder decode kernels:", sorted(set(_kinds(ops))))
        monkeypatch.setattr(ops, "PROFILE", None)
    assert bool(torch.isfinite(res[True]).all())
    close(res[True], res[False], rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------------------ B.3: weights beyond the weight scale
_BIG3 = "model.enc.32x32_block0.conv0.weight"      # 3x3, fed by a GroupNorm: fp16 format at 32x32 from B = 2
_BIG1 = "model.dec.32x32_block0.skip.weight"       # 1x1 behind a concatenation: fp16 format from 2048 pixels


def _bench_model(gpu):
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    import bench
    return bench.build_model(gpu)


def _plant(sd_or_params):
    """One 3x3 corner tap (U[0][0] of the Winograd weight = g[0][0]) and one 1x1 weight at 40: 40 * 2^11 leaves the fp16 range."""
    with torch.no_grad():
        for k, p in sd_or_params:
            if k.endswith(_BIG3):
                p[0, 0, 0, 0] = 40.0
            if k.endswith(_BIG1):
                p[0, 0, 0, 0] = 40.0


def test_weights_beyond_the_fp16_weight_scale_after_load_state_dict(ops, monkeypatch):
    """load_state_dict of weights with a 3x3 corner tap and a 1x1 weight at 40, then a forward and a 2-step sample(): finite and equal
    to the f32-MFMA path; the two layers run on the bf16 format, the others stay on the fp16 format."""
    gpu = torch.device("cuda:0")
    sd = {k: v.detach().cpu().clone() for k, v in _bench_model(gpu).state_dict().items()}
    _plant(sd.items())
    x = fill.hash_tensor((2, 3, 32, 32), "wx", 1.0).to(gpu)
    sigma = torch.tensor([0.3, 0.8], device=gpu)
    xT = fill.hash_tensor((2, 3, 32, 32), "wxT", 1.7, torch.float64).to(gpu)
    res = {}
    for mode in ("h3", "f32"):
        monkeypatch.setattr(ops, "BF16X6", mode == "h3")
        dpm = _bench_model(gpu).eval()
        dpm.load_state_dict(sd)
        dpm.sampling_timesteps = 2
        monkeypatch.setattr(ops, "PROFILE", [])
        with torch.no_grad():
            out = dpm.model(x, sigma)
        kinds = _h3_kinds(ops)
        monkeypatch.setattr(ops, "PROFILE", None)
        img = dpm.sample(batch_size=2, x_T=xT)
        outs = [o.detach().clone() for o in (out if isinstance(out, tuple) else (out,))] + [img.detach().clone()]
        for o in outs:
            assert bool(torch.isfinite(o).all()), mode
        if mode == "h3":
            assert {"wino2h3", "gemmh3"} <= kinds, kinds
            named = dict(dpm.named_parameters())
            for k, p in named.items():
                if k.endswith(_BIG3) or k.endswith(_BIG1):
                    assert p._adm_packed.h3_off, k
            assert sum(1 for p in named.values() if getattr(getattr(p, "_adm_packed", None), "w2fh", None) is not None) >= 8
        res[mode] = outs
    for a, b in zip(res["h3"], res["f32"]):
        close(a, b, rtol=1e-4, atol=1e-5)


def test_weights_beyond_the_fp16_weight_scale_in_a_training_step(ops, monkeypatch):
    """One optimiser step of the bench model with the same two weights at 40: loss and gradients finite and equal to the f32-MFMA
    path."""
    from adm_amd.optim import FlatParams, FusedAdamWEMA
    gpu = torch.device("cuda:0")
    B = 8
    g = torch.Generator().manual_seed(5)
    batch = {"image": (torch.rand(B, 3, 32, 32, generator=g) * 2 - 1).to(gpu)}
    t = (torch.rand(B, generator=g) * 0.999 + 0.001).to(gpu)
    noise = torch.randn(B, 3, 32, 32, generator=g).to(gpu)
    res = {}
    for mode in ("h3", "f32"):
        monkeypatch.setattr(ops, "BF16X6", mode == "h3")
        monkeypatch.setattr(ops, "_drop_counter", itertools.count(1))
        dpm = _bench_model(gpu).train()
        _plant(dpm.named_parameters())
        flat = FlatParams(dpm)
        opt = FusedAdamWEMA(flat, lr=1e-4, weight_decay=1e-4, max_norm=1.0, ema=True)
        flat.zero_grad()
        monkeypatch.setattr(ops, "PROFILE", [])
        loss, _ = dpm.training_step(batch, t=t, noise=noise)
        loss.backward()
        kinds = _h3_kinds(ops)
        monkeypatch.setattr(ops, "PROFILE", None)
        opt.step(lr=1e-4, grad_scale=1.0, ema_decay=0.999)
        torch.cuda.synchronize()
        assert math.isfinite(float(loss)) and bool(torch.isfinite(flat.grad).all()) and bool(torch.isfinite(flat.flat).all()), mode
        if mode == "h3":
            assert {"wino2h3", "gemmh3", "wgrad_wino2h3"} <= kinds, kinds
        res[mode] = (float(loss), flat.grad.clone(), flat.flat.clone())
    assert abs(res["h3"][0] - res["f32"][0]) <= 1e-5 * abs(res["f32"][0]), (res["h3"][0], res["f32"][0])
    gmax = float(res["f32"][1].abs().max())
    assert float((res["h3"][1] - res["f32"][1]).abs().max()) <= 1e-3 * gmax
    close(res["h3"][2], res["f32"][2], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ C: streams and pool refills
def _train_steps(ops, gpu, steps, B, seed=3):
    from adm_amd.optim import FlatParams, FusedAdamWEMA
    ops._drop_counter = itertools.count(1)
    dpm = _bench_model(gpu).train()
    flat = FlatParams(dpm)
    opt = FusedAdamWEMA(flat, lr=1e-4, weight_decay=1e-4, max_norm=1.0, ema=True)
    g = torch.Generator().manual_seed(seed)
    losses = []
    for _ in range(steps):
        batch = {"image": (torch.rand(B, 3, 32, 32, generator=g) * 2 - 1).to(gpu)}
        t = (torch.rand(B, generator=g) * 0.999 + 0.001).to(gpu)
        noise = torch.randn(B, 3, 32, 32, generator=g).to(gpu)
        flat.zero_grad()
        loss, _ = dpm.training_step(batch, t=t, noise=noise)
        loss.backward()
        opt.step(lr=1e-4, grad_scale=1.0, ema_decay=0.999)
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    return losses, flat


def test_bound_pools_are_ordered_and_held_by_every_stream_that_uses_them(ops, monkeypatch):
    """Audit of the bound-vector pools over one training step of the bench model with the side-stream weight gradients and the
    second decoder's stream on, and pools of 8 vectors (refills inside the branch-stream forward and the side-stream backward).
    Recorded: the stream each pool is created (zero-filled) on, the stream of every launch with a pointer into a pool, every
    wait_event and every record_stream.  Invariant: a stream that launches on a pool it was not created on has waited for the
    pool's zero-fill event before its first such launch, and holds a record_stream mark on the pool."""
    from adm_amd import hip
    monkeypatch.setattr(ops, "_AMAX_POOL", 8)
    monkeypatch.setattr(ops, "PROFILE", None)
    monkeypatch.setattr(ops, "SIDE_WGRAD", True)
    monkeypatch.setattr(ops, "BRANCH_STREAM", True)
    ops.new_amax_pool()
    seq = itertools.count()
    pools, launches, waits, marks = [], [], [], []
    cur = lambda: torch.cuda.current_stream().cuda_stream
    orig_slot, orig_call = ops._amax_slot, ops.call

    def slot(like):
        before = ops._amax_pool
        s = orig_slot(like)
        if ops._amax_pool is not before:
            p = ops._amax_pool
            pools.append((p.data_ptr(), p.data_ptr() + 4 * p.numel(), cur(), getattr(p, "_adm_fill", None), next(seq)))
        return s

    def call(name, *args):
        ptrs = [a.value for a in args if isinstance(a, ctypes.c_void_p) and a.value]
        for i in range(len(pools) - 1, -1, -1):      # the newest pool at an address (a freed pool's memory may hold a newer one)
            lo, hi = pools[i][0], pools[i][1]
            if any(lo <= q < hi for q in ptrs):
                launches.append((i, cur(), next(seq), name))
                break
        return orig_call(name, *args)

    orig_wait, orig_rec = torch.cuda.Stream.wait_event, torch.Tensor.record_stream

    def wait_event(self, event):
        waits.append((self.cuda_stream, event, next(seq)))
        return orig_wait(self, event)

    def record_stream(self, stream):
        marks.append((self.data_ptr(), stream.cuda_stream, next(seq)))
        return orig_rec(self, stream)

    monkeypatch.setattr(ops, "_amax_slot", slot)
    monkeypatch.setattr(ops, "call", call)
    monkeypatch.setattr(torch.cuda.Stream, "wait_event", wait_event)
    monkeypatch.setattr(torch.Tensor, "record_stream", record_stream)
    _train_steps(ops, torch.device("cuda:0"), 1, 16)
    monkeypatch.undo()
    ops.new_amax_pool()
    assert len({p[2] for p in pools}) >= 2, "no pool was created on the second decoder's stream"
    assert ops._side_stream is not None
    side = ops._side_stream.cuda_stream
    first = {}
    for i, s, n, name in launches:
        first.setdefault((i, s), (n, name))
    assert any(s == side for (_, s) in first), "the side stream read no bound"
    bad = []
    for (i, s), (n, name) in sorted(first.items()):
        lo, hi, s0, fill_ev, _ = pools[i]
        if s == s0:
            continue
        ordered = fill_ev is not None and any(ws == s and ev is fill_ev and wn < n for ws, ev, wn in waits)
        held = any(ms == s and lo <= mp < hi for mp, ms, _ in marks)
        if not (ordered and held):
            bad.append((i, hex(s0), hex(s), name, ordered, held))
    assert not bad, f"{len(bad)} (pool, stream) pairs used without ordering / lifetime mark, e.g. {bad[:6]}"


def test_deterministic_streams_and_pool_refills_are_bit_identical(ops, monkeypatch):
    """ADM_DETERMINISTIC with the side and branch streams on and pools of 8 vectors: three optimiser steps of the bench model give the
    same losses, flat gradient and parameters, bit for bit, as one stream with the default pool."""
    gpu = torch.device("cuda:0")
    monkeypatch.setattr(ops, "DETERMINISTIC", True)
    monkeypatch.setattr(ops, "PROFILE", None)
    res = {}
    for streams in (True, False):
        monkeypatch.setattr(ops, "SIDE_WGRAD", streams)
        monkeypatch.setattr(ops, "BRANCH_STREAM", streams)
        monkeypatch.setattr(ops, "_AMAX_POOL", 8 if streams else 4096)
        ops.new_amax_pool()
        losses, flat = _train_steps(ops, gpu, 3, 16)
        res[streams] = (torch.stack(losses).cpu(), flat.grad.clone(), flat.flat.clone())
    ops.new_amax_pool()
    assert bool(torch.isfinite(res[True][0]).all())
    assert torch.equal(res[True][0], res[False][0]), (res[True][0], res[False][0])
    assert torch.equal(res[True][1], res[False][1]), float((res[True][1] - res[False][1]).abs().max())
    assert torch.equal(res[True][2], res[False][2]), float((res[True][2] - res[False][2]).abs().max())


def test_loss_trajectory_fp16_format_vs_f32_mfma(ops, monkeypatch):
    """12 optimiser steps of the bench model at bs = 128 on the fixed batch stream of tools/loss_trajectory.py, default streams and
    formats: every loss finite and equal, to 1e-5 relative, to the same run on the f32-MFMA kernels on one stream."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from loss_trajectory import trajectory
    monkeypatch.setattr(ops, "PROFILE", None)
    res = {}
    for mode in ("h3", "f32"):
        monkeypatch.setattr(ops, "BF16X6", mode == "h3")
        monkeypatch.setattr(ops, "SIDE_WGRAD", mode == "h3")
        monkeypatch.setattr(ops, "BRANCH_STREAM", mode == "h3")
        monkeypatch.setattr(ops, "_drop_counter", itertools.count(1))
        res[mode] = trajectory(12, 128)
    print("fp16 format:", " ".join(f"{v:.7f}" for v in res["h3"]))
    print("f32 MFMA:   ", " ".join(f"{v:.7f}" for v in res["f32"]))
    assert all(math.isfinite(v) for v in res["h3"]), res["h3"]
    for a, b in zip(res["h3"], res["f32"]):
        assert abs(a - b) <= 1e-5 * abs(b), (res["h3"], res["f32"])
