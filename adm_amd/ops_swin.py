"""Forward-only operators of the Swin condition encoder over the HIP C ABI (csrc/swin.hip): what
/root/reference/unet/swin_transformer.py needs beyond ``adm_amd.ops`` / ``adm_amd.ops_cond``.  NHWC fp32 CUDA tensors, no autograd
Function (the encoder is frozen in this build: its backward pass is not built), no CPU / eager fallback.
"""
from __future__ import annotations

import torch

from .hip import call, ptr
from .ops import _chk, _new

WINDOW = 7
HEAD_DIM = 32


def relative_position_index() -> torch.Tensor:
    """flat [49 * 49] long: (dy + 6) * 13 + (dx + 6), (dy, dx) = query - key position in the window -- the formula the attention
    kernel evaluates in place of the reference's buffer (swin_transformer.py:207-219)."""
    p = torch.arange(WINDOW * WINDOW)
    y, x = p // WINDOW, p % WINDOW
    return ((y[:, None] - y[None, :] + WINDOW - 1) * (2 * WINDOW - 1) + (x[:, None] - x[None, :] + WINDOW - 1)).reshape(-1)


def window_attention(qkv, qkv_bias, table, heads: int, shift, window: int = WINDOW):
    """shifted_window_attention (swin_transformer.py:71-168) between its two Linears.  qkv [B, H, W, 3C] is the qkv Linear's output
    (bias included), ``table`` the [169, heads] relative_position_bias_table, ``shift`` an int or (shift_h, shift_w); returns
    [B, H, W, C].  Padding to multiples of 7, the roll, the partition, the bias, the -100 mask and their inverses happen inside the
    kernel; the shift of an axis that is a single window is switched off per call."""
    qkv = _chk(qkv, "qkv")
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    sh, sw = (shift, shift) if isinstance(shift, int) else shift
    qb, tb = _chk(qkv_bias.detach(), "qkv_bias"), _chk(table.detach(), "table")
    if C3 != 3 * C or qb.numel() != C3 or tuple(tb.shape) != ((2 * window - 1) ** 2, heads):
        raise RuntimeError(f"window_attention: qkv {tuple(qkv.shape)}, bias {tuple(qb.shape)}, table {tuple(tb.shape)}, {heads} heads")
    out = _new((B, H, W, C), qkv)
    call("adm_swin_attn_fwd", ptr(qkv), ptr(qb), ptr(tb), ptr(out), B, H, W, C, int(heads), int(window), int(sh), int(sw))
    return out


def layer_norm(x, weight, bias, eps: float = 1e-5):
    """nn.LayerNorm over the last axis (32..2048 entries) with weight and bias."""
    x = _chk(x, "x")
    C = x.shape[-1]
    w, b = _chk(weight.detach(), "weight"), _chk(bias.detach(), "bias")
    if w.numel() != C or b.numel() != C:
        raise RuntimeError(f"LayerNorm parameters have {w.numel()} / {b.numel()} entries, the rows {C}")
    y = _new(tuple(x.shape), x)
    call("adm_ln_affine_fwd", ptr(x), ptr(w), ptr(b), ptr(y), x.numel() // C, C, float(eps))
    return y


def merge_layer_norm(x, weight, bias, eps: float = 1e-5):
    """PatchMerging's pad + gather + LayerNorm(4C) (swin_transformer.py:58-66): [B, H, W, C] -> [B, ceil(H/2), ceil(W/2), 4C]."""
    x = _chk(x, "x")
    B, H, W, C = x.shape
    w, b = _chk(weight.detach(), "weight"), _chk(bias.detach(), "bias")
    if w.numel() != 4 * C or b.numel() != 4 * C:
        raise RuntimeError(f"PatchMerging norm has {w.numel()} entries, expected {4 * C}")
    y = _new((B, (H + 1) // 2, (W + 1) // 2, 4 * C), x)
    call("adm_swin_merge_ln_fwd", ptr(x), ptr(w), ptr(b), ptr(y), B, H, W, C, float(eps))
    return y


_ONE: dict = {}


def nhwc_to_nchw(x):
    """[B, H, W, C] -> [B, C, H, W] (the stage outputs the denoiser receives): the transposing store of the preconditioning
    kernel with a unit scale and no skip term."""
    x = _chk(x, "x")
    B, H, W, C = x.shape
    one = _ONE.get(x.device)
    if one is None:
        one = _ONE[x.device] = torch.ones(1, device=x.device, dtype=torch.float32)
    out = _new((B, C, H, W), x)
    call("adm_precond_out", None, 0, ptr(x), C, None, ptr(one), 0, ptr(out), B, C, H * W)
    return out
