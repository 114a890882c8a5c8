"""Autograd operators for TRAINING the KL autoencoder (ddm/encoder_decoder.py AutoencoderKL.training_step with ddm/loss.py
LPIPSWithDiscriminator) over the HIP C ABI: what the step needs beyond ``adm_amd.ops`` / ``adm_amd.ops_cond``.  Same conventions:
NHWC fp32 CUDA tensors with channels padded to multiples of 32, parameters in the reference's layouts, every backward a HIP kernel
(csrc/ae_train.hip plus the existing GEMM entry points), no CPU / eager fallback.  ``ops.conv2d_strided`` and ``ops.matmul_nt`` stay
forward-only; the differentiable forms live here under their own names.
"""
from __future__ import annotations

import torch

from . import hip, ops
from .hip import call, ptr
from .ops import _chk, _like, _new, _Prof, ceil32, packed


def _part(n_doubles: int, like):
    return _new((max(int(n_doubles), 1),), like, torch.float64)


# ------------------------------------------------------------------------------------------------ Downsample conv
class _ConvDown(torch.autograd.Function):
    """ops.conv2d_strided with a backward: ops._conv_wgrad_strided and ops._conv_dgrad_strided, as ops_cond._ConvGeneric -- plus the
    packed-weight cache of ops.packed() and, under ADM_DETERMINISTIC=1, a weight gradient without float atomics."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad_lo, pad_hi):
        x = _chk(x, "x")
        pk = packed(weight, bias, weight.shape[-1], False)
        y = ops._conv_fwd_strided(x, weight, pk.fwd, pk.bias, stride, pad_lo, pad_hi, f"fwd-s{stride}")
        ctx.save_for_backward(x, weight, bias)
        ctx.meta = (stride, pad_lo)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias = ctx.saved_tensors
        stride, pad_lo = ctx.meta
        dy = _chk(dy, "dy")
        dx = dw = db = None
        if ctx.needs_input_grad[1]:
            dw, db = ops._conv_wgrad_strided(x, dy, weight, bias, bias is not None and ctx.needs_input_grad[2], stride, pad_lo, True)
        if ctx.needs_input_grad[0]:
            dx = ops._conv_dgrad_strided(dy, weight, x.shape, stride, pad_lo)
        return dx, dw, db, None, None, None


def conv2d_down(x, weight, bias=None, *, stride=2, pad_lo=0, pad_hi=1):
    """The differentiable form of ops.conv2d_strided (filter size up to 7 from the weight): the autoencoder's Downsample =
    F.pad(x, (0,1,0,1)) + Conv2d(3x3, stride 2, padding 0) (encoder_decoder.py:78-96) is stride=2, pad_lo=0, pad_hi=1; the PatchGAN
    discriminator's Conv2d(4x4, stride s, padding 1) is stride=s, pad_lo=pad_hi=1."""
    return _ConvDown.apply(x, weight, bias, int(stride), int(pad_lo), int(pad_hi))


# ------------------------------------------------------------------------------------------------ single-head attention core
def _nt(a, b, out, bias=None):
    """out[M][N] = sum_k a[m][k] b[n][k] (+ bias[n]) on the implicit-GEMM kernel."""
    return ops._mm_nt(a, b, bias, out)


def _tn(a, b, out):
    """out[N][K] = sum_m a[m][n] b[m][k]: the 1x1 weight-gradient kernel with a as dy and b as x; one pixel range, so no atomics."""
    M, N = a.shape
    K = b.shape[1]
    with _Prof("wgrad", 2.0 * M * N * K, f"mm-tn P={M} Co={N} Ci={K}"):
        call("adm_conv_wgrad", ptr(b), ptr(a), ptr(out), 1, M, 1, K, K, N, N, 1, 0, 1)
    return out


def _transpose(x, out):
    call("adm_transpose2d", ptr(x), ptr(out), x.shape[0], x.shape[1])
    return out


class _AttnCore(torch.autograd.Function):
    """softmax(C^-1/2 q k^T) v per image with one head of width C (AttnBlock, encoder_decoder.py:169-213); q, k, v [B, L, C].
    The [L, L] scores live in HBM one image at a time; the backward recomputes P from q and k instead of keeping it."""

    @staticmethod
    def _probs(q, k, s, scale):
        _nt(q, k, s)
        call("adm_softmax_rows", ptr(s), s.shape[0], s.shape[1], s.shape[1], float(scale))
        return s

    @staticmethod
    def forward(ctx, q, k, v):
        q, k, v = _chk(q, "q"), _chk(k, "k"), _chk(v, "v")
        B, L, C = q.shape
        if C % 32 or L % 32:
            raise RuntimeError(f"attention needs C ({C}) and L ({L}) to be multiples of 32")
        scale = float(C) ** -0.5
        o = _like(q)
        s = _new((L, L), q)
        vt = _new((C, L), q)
        for b in range(B):
            _AttnCore._probs(q[b], k[b], s, scale)
            _transpose(v[b], vt)
            _nt(s, vt, o[b])
        ctx.save_for_backward(q, k, v)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v = ctx.saved_tensors
        do = _chk(do, "do")
        B, L, C = q.shape
        scale = float(C) ** -0.5
        dq, dk, dv = _like(q), _like(k), _like(v)
        s = _new((L, L), q)
        dp = _new((L, L), q)
        kt = _new((C, L), q)
        for b in range(B):
            _AttnCore._probs(q[b], k[b], s, scale)
            _tn(s, do[b], dv[b])                         # dV = P^T dO
            _nt(do[b], v[b], dp)                         # dP = dO V^T
            call("adm_softmax_rows_bwd", ptr(s), ptr(dp), L, L, L, scale)      # dS, in place on dP
            _transpose(k[b], kt)
            _nt(dp, kt, dq[b])                           # dQ = dS K
            _tn(dp, q[b], dk[b])                         # dK = dS^T Q
        return dq, dk, dv


def attention_single_head(q, k, v):
    return _AttnCore.apply(q, k, v)


# ------------------------------------------------------------------------------------------------ posterior sample + KL
class _PosteriorKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, moments, eps, C, ldz):
        moments, eps = _chk(moments, "moments"), _chk(eps, "eps")
        B, H, W, ld = moments.shape
        if tuple(eps.shape) != (B, H, W, C):
            raise RuntimeError(f"eps is {tuple(eps.shape)}, expected {(B, H, W, C)}")
        z = _new((B, H, W, ldz), moments)
        kl = _new((B,), moments)
        part = _part(B * hip.lib().adm_ae_blocks(H * W * ldz), moments)
        call("adm_posterior_kl_fwd", ptr(moments), ld, ptr(eps), ptr(z), ldz, ptr(kl), ptr(part), B, H * W, C)
        ctx.save_for_backward(moments, eps)
        ctx.C = C
        ctx.set_materialize_grads(False)
        return z, kl

    @staticmethod
    def backward(ctx, dz, dkl):
        moments, eps = ctx.saved_tensors
        B, H, W, ld = moments.shape
        dz = None if dz is None else _chk(dz, "dz")
        dkl = None if dkl is None else _chk(dkl, "dkl")
        dm = _like(moments)
        call("adm_posterior_kl_bwd", ptr(moments), ld, ptr(eps), ptr(dz), 0 if dz is None else dz.shape[-1], ptr(dkl), ptr(dm), B,
             H * W, ctx.C)
        return dm, None, None, None


def posterior_sample_kl(moments, C: int, eps, ldz: int = 0):
    """moments NHWC [B,H,W,>=2C] (mean | logvar), eps NHWC [B,H,W,C] -> (z NHWC [B,H,W,ldz] with zero pad channels, kl [B]):
    DiagonalGaussianDistribution.sample and .kl (encoder_decoder.py:854-892) with their gradients to the moments."""
    return _PosteriorKL.apply(moments, eps, int(C), int(ldz) if ldz else ceil32(C))


# ------------------------------------------------------------------------------------------------ reconstruction / NLL
class _Nll(torch.autograd.Function):
    """out [4] = (nll_loss, rec_loss, d nll / d logvar, exp(-logvar) / B) of adm_ae_nll_fwd; only out[0] is differentiable:
    with respect to the reconstruction, the LPIPS values and logvar."""

    @staticmethod
    def forward(ctx, x, r, p, logvar, pw):
        x, r = _chk(x, "inputs"), _chk(r, "reconstructions")
        if x.shape != r.shape:
            raise RuntimeError(f"inputs {tuple(x.shape)} and reconstructions {tuple(r.shape)} differ")
        B = x.shape[0]
        n_per = x.numel() // B
        pp = None if p is None else _chk(p.reshape(-1), "p_loss")
        lv = _chk(logvar.detach().reshape(1), "logvar")
        out = _new((4,), x)
        part = _part(hip.lib().adm_ae_blocks(x.numel()), x)
        call("adm_ae_nll_fwd", ptr(x), ptr(r), ptr(pp), ptr(lv), ptr(out), ptr(part), B, n_per, float(pw))
        ctx.save_for_backward(x, r, out)
        ctx.meta = (B, n_per, float(pw), None if p is None else tuple(p.shape), tuple(logvar.shape))
        return out

    @staticmethod
    def backward(ctx, dout):
        x, r, out = ctx.saved_tensors
        B, n_per, pw, pshape, lvshape = ctx.meta
        dout = _chk(dout, "dout")
        dr = dp = dlv = None
        gs = (dout[0] * out[3]).reshape(1)         # d loss / d (one element of rec_loss): a device scalar, never read back
        if ctx.needs_input_grad[1]:
            dr = _like(r)
            call("adm_ae_nll_bwd", ptr(x), ptr(r), ptr(gs), 1.0, ptr(dr), x.numel())
        if pshape is not None and ctx.needs_input_grad[2]:
            dp = (gs * (pw * n_per)).expand(B).reshape(pshape).contiguous()
        if ctx.needs_input_grad[3]:
            dlv = (dout[0] * out[2]).reshape(lvshape)
        return None, dr, dp, dlv, None


def nll_terms(inputs, reconstructions, p_loss, logvar, perceptual_weight: float = 1.0):
    """(nll_loss, rec_loss) of LPIPSWithDiscriminator.forward as a [4] vector (see _Nll); p_loss [B] or None."""
    return _Nll.apply(inputs, reconstructions, p_loss, logvar, float(perceptual_weight))


# ------------------------------------------------------------------------------------------------ hinge / generator terms
class _LogitTerm(torch.autograd.Function):
    """One mean over the logit map [B,H,W,32] (channel 0 real): mode 0 relu(1 - l), 1 relu(1 + l), 2 l.  The pad channels take no
    part and receive zero gradient."""

    @staticmethod
    def forward(ctx, logits, mode):
        logits = _chk(logits, "logits")
        ld = logits.shape[-1]
        M = logits.numel() // ld
        out = _new((3,), logits)
        part = _part(3 * hip.lib().adm_ae_blocks(M), logits)
        call("adm_logit_terms_fwd", ptr(logits), ld, ptr(out), ptr(part), M)
        ctx.save_for_backward(logits)
        ctx.mode = mode
        return out[mode].clone()

    @staticmethod
    def backward(ctx, dout):
        (logits,) = ctx.saved_tensors
        ld = logits.shape[-1]
        dl = _like(logits)
        call("adm_logit_terms_bwd", ptr(logits), ld, ctx.mode, ptr(_chk(dout.reshape(1), "dout")), 1.0, ptr(dl), logits.numel() // ld)
        return dl, None


def hinge_real(logits):
    return _LogitTerm.apply(logits, 0)


def hinge_fake(logits):
    return _LogitTerm.apply(logits, 1)


def logit_mean(logits):
    return _LogitTerm.apply(logits, 2)


# ------------------------------------------------------------------------------------------------ LeakyReLU
class _LeakyRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slope):
        x = _chk(x, "x")
        y = _like(x)
        call("adm_leaky_relu_fwd", ptr(x), ptr(y), x.numel(), float(slope))
        ctx.save_for_backward(x)
        ctx.slope = slope
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dx = _like(x)
        call("adm_leaky_relu_bwd", ptr(x), ptr(_chk(dy, "dy")), ptr(dx), x.numel(), float(ctx.slope))
        return dx, None


def leaky_relu(x, slope: float = 0.2):
    return _LeakyRelu.apply(x, float(slope))


# ------------------------------------------------------------------------------------------------ adaptive weight
def adaptive_weight(nll_grads, g_grads, disc_weight: float):
    """clamp(|nll_grads| / (|g_grads| + 1e-4), 0, 1e4) * disc_weight as a device scalar (calculate_adaptive_weight, loss.py)."""
    a, b = _chk(nll_grads.detach(), "nll_grads"), _chk(g_grads.detach(), "g_grads")
    lib = hip.lib()
    part = _part(lib.adm_ae_blocks(a.numel()) + lib.adm_ae_blocks(b.numel()), a)
    out = _new((1,), a)
    call("adm_adaptive_weight", ptr(a), a.numel(), ptr(b), b.numel(), ptr(part), float(disc_weight), ptr(out))
    return out.reshape(())


def axpy_dev(a, b, coef, mul: float = 1.0):
    """a + coef * mul * b with coef a device scalar (the adaptive weight): the combined gradient at the decoder's output."""
    a, b = _chk(a, "a"), _chk(b, "b")
    if a.shape != b.shape:
        raise RuntimeError(f"shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    out = _like(a)
    call("adm_axpy_dev", ptr(a), ptr(b), ptr(_chk(coef.detach().reshape(1), "coef")), float(mul), ptr(out), a.numel())
    return out
