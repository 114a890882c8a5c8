"""Operators of the Swin condition encoder over the HIP C ABI (csrc/swin.hip): what /root/reference/unet/swin_transformer.py needs
beyond ``adm_amd.ops`` / ``adm_amd.ops_cond``.  NHWC fp32 CUDA tensors, no CPU / eager fallback.  ``window_attention``,
``layer_norm``, ``merge_layer_norm`` and ``nhwc_to_nchw`` are autograd Functions with HIP backward kernels; when nothing
requires grad (the frozen encoder: its forward runs under no_grad) they are the plain forward launches they always were.
``row_scale_add`` is stochastic depth in "row" mode.  ``patch_embed_ln`` is the stem of the single-channel encoder (4x4 stride-4
conv of a one-channel image + LayerNorm in one kernel; parameter gradients only).  The training path is f32 only: in the bf16 compute mode it raises.
"""
from __future__ import annotations

import torch

from . import hip, ops
from .hip import call, ptr
from .ops import _chk, _direct_grad, _mark_uses, _new, _notify

WINDOW = 7
HEAD_DIM = 32


def relative_position_index() -> torch.Tensor:
    """flat [49 * 49] long: (dy + 6) * 13 + (dx + 6), (dy, dx) = query - key position in the window -- the formula the attention
    kernel evaluates in place of the reference's buffer (swin_transformer.py:207-219)."""
    p = torch.arange(WINDOW * WINDOW)
    y, x = p // WINDOW, p % WINDOW
    return ((y[:, None] - y[None, :] + WINDOW - 1) * (2 * WINDOW - 1) + (x[:, None] - x[None, :] + WINDOW - 1)).reshape(-1)


def _wants_grad(*tensors) -> bool:
    if not torch.is_grad_enabled() or not any(t is not None and t.requires_grad for t in tensors):
        return False
    if ops.COMPUTE != "f32":
        raise NotImplementedError("the Swin condition encoder trains in the f32 compute mode only (bf16 mode is not implemented)")
    return True


def _param_grad(param, want: bool):
    """(destination, accumulate) of a parameter gradient: the parameter's slice of the flat gradient buffer when
    adm_amd.optim.FlatParams owns it (the kernel then adds to it), else a fresh tensor that autograd accumulates."""
    if not want:
        return torch.empty_like(param), False          # the kernels always write both: a scratch destination
    sink = _direct_grad(param)
    return (sink, True) if sink is not None else (torch.empty_like(param), False)


def _hand_over(param, dst, want: bool, direct: bool):
    """What backward returns for a parameter: None when the kernel accumulated in place (announced through ops._notify)."""
    if not want:
        return None
    if direct:
        _notify(param)
        return None
    return dst


def _attn_args(qkv, qkv_bias, table, heads, window):
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    if C3 != 3 * C or qkv_bias.numel() != C3 or tuple(table.shape) != ((2 * window - 1) ** 2, heads):
        raise RuntimeError(f"window_attention: qkv {tuple(qkv.shape)}, bias {tuple(qkv_bias.shape)}, table {tuple(table.shape)}, {heads} heads")
    return B, H, W, C


def _window_attention(qkv, qb, tb, heads, sh, sw, window):
    B, H, W, C = _attn_args(qkv, qb, tb, heads, window)
    out = _new((B, H, W, C), qkv)
    call("adm_swin_attn_fwd", ptr(qkv), ptr(qb), ptr(tb), ptr(out), B, H, W, C, int(heads), int(window), int(sh), int(sw))
    return out


class _WindowAttention(torch.autograd.Function):
    """Saves its three inputs only: the backward kernel recomputes scores and softmax."""

    @staticmethod
    def forward(ctx, qkv, qkv_bias, table, heads, sh, sw, window):
        qkv = _chk(qkv, "qkv")
        out = _window_attention(qkv, _chk(qkv_bias.detach(), "qkv_bias"), _chk(table.detach(), "table"), heads, sh, sw, window)
        ctx.save_for_backward(qkv, qkv_bias, table)
        _mark_uses(ctx, (1, qkv_bias), (2, table))
        ctx.meta = (heads, sh, sw, window)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, qkv_bias, table = ctx.saved_tensors
        heads, sh, sw, window = ctx.meta
        dout = _chk(dout, "dout")
        B, H, W, C3 = qkv.shape
        C = C3 // 3
        d_qkv = _new(tuple(qkv.shape), qkv)
        ws = _new((hip.lib().adm_swin_attn_bwd_ws_floats(B, H, W, int(heads)),), qkv)
        want_b, want_t = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        db, acc_b = _param_grad(qkv_bias, want_b)
        dt, acc_t = _param_grad(table, want_t)
        call("adm_swin_attn_bwd", ptr(qkv), ptr(_chk(qkv_bias.detach(), "qkv_bias")), ptr(_chk(table.detach(), "table")), ptr(dout),
             ptr(d_qkv), ptr(dt), ptr(db), ptr(ws), B, H, W, C, int(heads), int(window), int(sh), int(sw), int(acc_t), int(acc_b))
        return (d_qkv if ctx.needs_input_grad[0] else None, _hand_over(qkv_bias, db, want_b, acc_b),
                _hand_over(table, dt, want_t, acc_t), None, None, None, None)


def window_attention(qkv, qkv_bias, table, heads: int, shift, window: int = WINDOW):
    """shifted_window_attention (swin_transformer.py:71-168) between its two Linears.  qkv [B, H, W, 3C] is the qkv Linear's output
    (bias included), ``table`` the [169, heads] relative_position_bias_table, ``shift`` an int or (shift_h, shift_w); returns
    [B, H, W, C].  Padding to multiples of 7, the roll, the partition, the bias, the -100 mask and their inverses happen inside the
    kernel; the shift of an axis that is a single window is switched off per call.  Differentiable in qkv, qkv_bias (the padding
    tokens' keys and values ARE the bias) and table."""
    sh, sw = (shift, shift) if isinstance(shift, int) else shift
    if _wants_grad(qkv, qkv_bias, table):
        return _WindowAttention.apply(qkv, qkv_bias, table, int(heads), int(sh), int(sw), int(window))
    return _window_attention(_chk(qkv, "qkv"), _chk(qkv_bias.detach(), "qkv_bias"), _chk(table.detach(), "table"), heads, sh, sw, window)


def _ln_params(weight, bias, C, what):
    w, b = _chk(weight.detach(), "weight"), _chk(bias.detach(), "bias")
    if w.numel() != C or b.numel() != C:
        raise RuntimeError(f"{what} has {w.numel()} / {b.numel()} entries, expected {C}")
    return w, b


def _layer_norm(x, w, b, eps):
    C = x.shape[-1]
    y = _new(tuple(x.shape), x)
    call("adm_ln_affine_fwd", ptr(x), ptr(w), ptr(b), ptr(y), x.numel() // C, C, float(eps))
    return y


def _merge_layer_norm(x, w, b, eps):
    B, H, W, C = x.shape
    y = _new((B, (H + 1) // 2, (W + 1) // 2, 4 * C), x)
    call("adm_swin_merge_ln_fwd", ptr(x), ptr(w), ptr(b), ptr(y), B, H, W, C, float(eps))
    return y


class _LayerNorm(torch.autograd.Function):
    """merge = PatchMerging's gather in front of the norm.  Saves x: the backward kernels recompute the row statistics."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, merge):
        x = _chk(x, "x")
        w, b = _ln_params(weight, bias, (4 if merge else 1) * x.shape[-1], "PatchMerging norm" if merge else "LayerNorm")
        y = (_merge_layer_norm if merge else _layer_norm)(x, w, b, eps)
        ctx.save_for_backward(x, weight, bias)
        _mark_uses(ctx, (1, weight), (2, bias))
        ctx.meta = (float(eps), merge)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias = ctx.saved_tensors
        eps, merge = ctx.meta
        dy = _chk(dy, "dy")
        C = dy.shape[-1]
        M = dy.numel() // C
        dx = _new(tuple(x.shape), x)
        ws = _new((hip.lib().adm_ln_bwd_ws_floats(M, C),), x)
        want_w, want_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dw, acc_w = _param_grad(weight, want_w)
        db, acc_b = _param_grad(bias, want_b)
        if acc_w != acc_b:                              # one flag for the pair: a lone sink goes through autograd
            if acc_w:
                dw, acc_w = torch.empty_like(weight), False
            else:
                db, acc_b = torch.empty_like(bias), False
        w = _chk(weight.detach(), "weight")
        if merge:
            B, H, W, Cin = x.shape
            call("adm_swin_merge_ln_bwd", ptr(x), ptr(w), ptr(dy), ptr(dx), ptr(dw), ptr(db), ptr(ws), B, H, W, Cin, eps, int(acc_w))
        else:
            call("adm_ln_affine_bwd", ptr(x), ptr(w), ptr(dy), ptr(dx), ptr(dw), ptr(db), ptr(ws), M, C, eps, int(acc_w))
        return (dx if ctx.needs_input_grad[0] else None, _hand_over(weight, dw, want_w, acc_w), _hand_over(bias, db, want_b, acc_b),
                None, None)


def layer_norm(x, weight, bias, eps: float = 1e-5):
    """nn.LayerNorm over the last axis (32..2048 entries) with weight and bias; differentiable in all three."""
    if _wants_grad(x, weight, bias):
        return _LayerNorm.apply(x, weight, bias, float(eps), False)
    x = _chk(x, "x")
    return _layer_norm(x, *_ln_params(weight, bias, x.shape[-1], "LayerNorm"), eps)


def merge_layer_norm(x, weight, bias, eps: float = 1e-5):
    """PatchMerging's pad + gather + LayerNorm(4C) (swin_transformer.py:58-66): [B, H, W, C] -> [B, ceil(H/2), ceil(W/2), 4C];
    differentiable in all three."""
    if _wants_grad(x, weight, bias):
        return _LayerNorm.apply(x, weight, bias, float(eps), True)
    x = _chk(x, "x")
    return _merge_layer_norm(x, *_ln_params(weight, bias, 4 * x.shape[-1], "PatchMerging norm"), eps)


def _patch_embed_args(x, conv_w, conv_b, ln_w, ln_b):
    if x.dim() != 4 or x.shape[1] != 1:
        raise RuntimeError(f"patch_embed_ln takes an NCHW image with 1 channel, got {tuple(x.shape)}")
    E = conv_w.shape[0]
    if tuple(conv_w.shape) != (E, 1, 4, 4) or any(t.numel() != E for t in (conv_b, ln_w, ln_b)):
        raise RuntimeError(f"patch_embed_ln: stem weight {tuple(conv_w.shape)} (expected [E, 1, 4, 4]), bias {tuple(conv_b.shape)}, "
                           f"norm {tuple(ln_w.shape)} / {tuple(ln_b.shape)}")
    B, _, H, W = x.shape
    return B, H, W, E


def _patch_embed_ln(x, cw, cb, lw, lb, eps):
    B, H, W, E = _patch_embed_args(x, cw, cb, lw, lb)
    y = _new((B, H // 4, W // 4, E), x)
    call("adm_patch_embed_ln_fwd", ptr(x), ptr(cw), ptr(cb), ptr(lw), ptr(lb), ptr(y), B, H, W, E, float(eps))
    return y


class _PatchEmbedLN(torch.autograd.Function):
    """Saves x and the four parameters: the backward kernel recomputes the conv outputs and the token statistics."""

    @staticmethod
    def forward(ctx, x, conv_w, conv_b, ln_w, ln_b, eps):
        params = (conv_w, conv_b, ln_w, ln_b)
        y = _patch_embed_ln(x, *(_chk(p.detach(), "parameter") for p in params), eps)
        ctx.save_for_backward(x, *params)
        _mark_uses(ctx, *((i + 1, p) for i, p in enumerate(params)))
        ctx.eps = float(eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, *params = ctx.saved_tensors
        dy = _chk(dy, "dy")
        B, H, W, E = _patch_embed_args(x, *params)
        want = [ctx.needs_input_grad[i + 1] for i in range(4)]
        sinks = [_param_grad(p, w) for p, w in zip(params, want)]
        ws = _new((hip.lib().adm_patch_embed_ln_bwd_ws_floats(B, H, W, E),), x)
        cw, cb, lw, _ = (_chk(p.detach(), "parameter") for p in params)
        call("adm_patch_embed_ln_bwd", ptr(x), ptr(cw), ptr(cb), ptr(lw), ptr(dy), *(ptr(d) for d, _ in sinks), ptr(ws), B, H, W, E,
             ctx.eps, sum(int(acc) << i for i, (_, acc) in enumerate(sinks)))
        return (None, *(_hand_over(p, d, w, acc) for p, w, (d, acc) in zip(params, want, sinks)), None)


def patch_embed_ln(x, conv_w, conv_b, ln_w, ln_b, eps: float = 1e-5):
    """Conv2d(1, E, 4, 4) + LayerNorm(E) of a one-channel NCHW image in one kernel: [B, 1, H, W] -> [B, H // 4, W // 4, E] NHWC
    (E a multiple of 32, at most 512; H, W >= 4).  Differentiable in the four parameters only: the condition image never takes a
    gradient, so an ``x`` that requires one is refused."""
    if x.requires_grad:
        raise RuntimeError("patch_embed_ln has no gradient for its input image (the condition takes none): detach it")
    x = _chk(x, "x")
    if _wants_grad(conv_w, conv_b, ln_w, ln_b):
        _patch_embed_args(x, conv_w, conv_b, ln_w, ln_b)
        return _PatchEmbedLN.apply(x, conv_w, conv_b, ln_w, ln_b, float(eps))
    return _patch_embed_ln(x, *(_chk(p.detach(), "parameter") for p in (conv_w, conv_b, ln_w, ln_b)), eps)


_ONE: dict = {}


def _nhwc_to_nchw(x):
    B, H, W, C = x.shape
    one = _ONE.get(x.device)
    if one is None:
        one = _ONE[x.device] = torch.ones(1, device=x.device, dtype=torch.float32)
    out = _new((B, C, H, W), x)
    call("adm_precond_out", None, 0, ptr(x), C, None, ptr(one), 0, ptr(out), B, C, H * W)
    return out


class _NhwcToNchw(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _nhwc_to_nchw(_chk(x, "x"))

    @staticmethod
    def backward(ctx, dy):
        dy = _chk(dy, "dy")
        B, C, H, W = dy.shape
        dx = _new((B, H, W, C), dy)
        call("adm_nchw_to_nhwc", ptr(dy), 0, None, 0, ptr(dx), B, C, H * W, C)          # the transposing store, the other way
        return dx


def nhwc_to_nchw(x):
    """[B, H, W, C] -> [B, C, H, W] (the stage outputs the denoiser receives): the transposing store of the preconditioning
    kernel with a unit scale and no skip term; its gradient is the opposite transpose."""
    if _wants_grad(x):
        return _NhwcToNchw.apply(x)
    return _nhwc_to_nchw(_chk(x, "x"))


def _row_scale_add(x, r, s):
    B = r.shape[0]
    y = _new(tuple(r.shape), r)
    call("adm_rowscale_add", ptr(x), ptr(r), ptr(s), ptr(y), B, r.numel() // B)
    return y


class _RowScaleAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r, s):
        ctx.save_for_backward(s)
        return _row_scale_add(x, r, s)

    @staticmethod
    def backward(ctx, dy):
        (s,) = ctx.saved_tensors
        dy = _chk(dy, "dy")
        return (dy if ctx.needs_input_grad[0] else None, _row_scale_add(None, dy, s) if ctx.needs_input_grad[1] else None, None)


def row_scale_add(x, r, s):
    """x + s[b] * r per sample b: stochastic depth in "row" mode, s[b] = keep_b / (1 - p) with keep_b ~ Bernoulli(1 - p) drawn
    by the caller.  torchvision.ops.StochasticDepth(p, "row"), which the reference wraps around both branches of a block
    (swin_transformer.py:292,303-304), is restated here from that use (torchvision is not a dependency): in training the branch
    of sample b is multiplied by keep_b / (1 - p); in eval, or with p == 0, it is the identity.  A dropped sample's output is x
    bit for bit.  s carries no gradient."""
    x, r = _chk(x, "x"), _chk(r, "r")
    s = _chk(s.detach().reshape(-1), "s")
    if x.shape != r.shape or s.numel() != r.shape[0] or (r.numel() // r.shape[0]) % 4:
        raise RuntimeError(f"row_scale_add: x {tuple(x.shape)}, r {tuple(r.shape)}, s {tuple(s.shape)} (per-sample size a multiple of 4)")
    if _wants_grad(x, r):
        return _RowScaleAdd.apply(x, r, s)
    return _row_scale_add(x, r, s)
