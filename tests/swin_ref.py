"""Plain-PyTorch CPU restatement of the Swin condition encoder (TEST INFRASTRUCTURE ONLY), in whatever dtype its inputs have
(the tests use fp64, and fp32 to measure the restatement's own noise).

Restated from the reference's unet/swin_transformer.py: PatchMerging :51-68, shifted_window_attention :71-168, the relative
position index :207-219 and the bias lookup :231-234, SwinTransformerBlock :302-305, the stem :363-369, the stage layout
:371-399 and forward :412-425.  The windowing is written as explicit index arithmetic (one gather of key/value tokens per
window) rather than as the reference's pad / roll / view chain, so that the two agree only if the arithmetic does.

It also holds the fill rule of the synthetic weights (hash-filled through oracle.fill.hash_tensor, so a golden file stores
outputs only) and the cases of tests/golden/g19_swin.npz.
"""
import math
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import fill

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_swin.npz")
WIN = 7
HEAD_DIM = 32

# attention alone: name -> (B, H, W, C, heads, shift)
ATTN_CASES = OrderedDict([
    ("a9x10", (2, 9, 10, 64, 2, 3)),        # pads to 14x14: 4 windows, all nine mask regions, bias-valued keys
    ("a7x15", (2, 7, 15, 64, 2, 3)),        # shift off on one axis only
    ("a14x14", (2, 14, 14, 32, 1, 0)),      # no padding, no mask
    ("a5x5", (2, 5, 5, 32, 1, 3)),          # one window, shift off on both axes, 24 of 49 keys are bias tokens
    ("a8x8", (1, 8, 8, 1024, 32, 3)),       # the last stage's head count
])
# PatchMerging: name -> (B, H, W, C)
MERGE_CASES = OrderedDict([("m9x11", (2, 9, 11, 64)), ("m4x6", (2, 4, 6, 32))])
SMALL = dict(embed_dim=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8))
SMALL_INPUT = (2, 3, 72, 88)
SWIN_B = dict(embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32))
SWIN_B_INPUTS = OrderedDict([("b64", (1, 3, 64, 64)), ("b112", (1, 3, 112, 112))])
SAMPLE_CAP = 4096


def sample(a):
    """What the golden file keeps of an array: every k-th element of the flattened array, k odd (so the walk visits every
    channel and every position), at most ~SAMPLE_CAP of them."""
    flat = a.reshape(-1)
    k = max(1, -(-flat.shape[0] // SAMPLE_CAP))
    k += 1 - (k & 1)
    return flat[::k]


# ------------------------------------------------------------------------------------------------ parameters
def relative_position_index():
    """flat [49 * 49]: (dy + 6) * 13 + (dx + 6) with (dy, dx) = query position - key position inside the window."""
    p = torch.arange(WIN * WIN)
    y, x = p // WIN, p % WIN
    dy, dx = y[:, None] - y[None, :], x[:, None] - x[None, :]
    return ((dy + WIN - 1) * (2 * WIN - 1) + (dx + WIN - 1)).reshape(-1)


def param_shapes(embed_dim, depths, num_heads, num_classes=1000):
    """state_dict() names and shapes of the reference's SwinTransformer, in its registration order."""
    s = OrderedDict()
    E = embed_dim
    s["first_coonv.0.weight"], s["first_coonv.0.bias"] = (E, 3, 4, 4), (E,)
    s["first_coonv.2.weight"], s["first_coonv.2.bias"] = (E,), (E,)
    for st, (d, nh) in enumerate(zip(depths, num_heads)):
        C = E * 2 ** st
        for i in range(d):
            p = f"features.{2 * st}.{i}."
            s[p + "norm1.weight"], s[p + "norm1.bias"] = (C,), (C,)
            s[p + "attn.relative_position_bias_table"] = ((2 * WIN - 1) ** 2, nh)
            s[p + "attn.relative_position_index"] = (WIN ** 4,)
            s[p + "attn.qkv.weight"], s[p + "attn.qkv.bias"] = (3 * C, C), (3 * C,)
            s[p + "attn.proj.weight"], s[p + "attn.proj.bias"] = (C, C), (C,)
            s[p + "norm2.weight"], s[p + "norm2.bias"] = (C,), (C,)
            s[p + "mlp.0.weight"], s[p + "mlp.0.bias"] = (4 * C, C), (4 * C,)
            s[p + "mlp.3.weight"], s[p + "mlp.3.bias"] = (C, 4 * C), (C,)
        if st < len(depths) - 1:
            p = f"features.{2 * st + 1}."
            s[p + "reduction.weight"] = (2 * C, 4 * C)
            s[p + "norm.weight"], s[p + "norm.bias"] = (4 * C,), (4 * C,)
    C = E * 2 ** (len(depths) - 1)
    s["norm.weight"], s["norm.bias"] = (C,), (C,)
    s["head.weight"], s["head.bias"] = (num_classes, C), (num_classes,)
    return s


def fill_value(name, shape, dtype=torch.float64):
    """The scale rule: Linear / conv weights 1/sqrt(fan_in), LayerNorm weights 1 +- 0.1, biases 0.1, the bias table 0.5."""
    leaf = name.rsplit(".", 1)[-1]
    if leaf == "relative_position_index":
        return relative_position_index()
    if leaf == "relative_position_bias_table":
        return fill.hash_tensor(shape, name, 0.5, dtype)
    if leaf == "bias":
        return fill.hash_tensor(shape, name, 0.1, dtype)
    if len(shape) == 1:                                        # every 1-D weight is a LayerNorm's
        return 1.0 + fill.hash_tensor(shape, name, 0.1, dtype)
    return fill.hash_tensor(shape, name, (1.0 / int(np.prod(shape[1:]))) ** 0.5, dtype)


def filled_state_dict(embed_dim, depths, num_heads, num_classes=1000, dtype=torch.float64):
    return OrderedDict((k, fill_value(k, s, dtype)) for k, s in param_shapes(embed_dim, depths, num_heads, num_classes).items())


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------ arithmetic
def _ceil(n, m):
    return -(-n // m) * m


def attn_core(qkv, qkv_bias, table, heads, shift):
    """The window attention between the qkv Linear and the proj Linear.  qkv [B, H, W, 3C] = Linear(x) with its bias, last
    axis ordered [3][heads][32]; returns [B, H, W, C].  Tokens outside H x W (the zero padding up to multiples of 7) are
    keys / values equal to qkv_bias; their own rows are never produced."""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    Ph, Pw = _ceil(H, WIN), _ceil(W, WIN)
    sh = shift if Ph > WIN else 0
    sw = shift if Pw > WIN else 0
    # source coordinate (padded frame) of every position of the rolled frame, and its region label along each axis
    ry, rx = torch.arange(Ph), torch.arange(Pw)
    sy, sx = (ry + sh) % Ph, (rx + sw) % Pw
    ly = torch.zeros(Ph, dtype=torch.long) if sh == 0 else (ry >= Ph - WIN).long() + (ry >= Ph - sh).long()
    lx = torch.zeros(Pw, dtype=torch.long) if sw == 0 else (rx >= Pw - WIN).long() + (rx >= Pw - sw).long()
    full = qkv_bias.to(qkv.dtype).expand(B, Ph, Pw, C3).clone()
    full[:, :H, :W] = qkv
    out = torch.zeros(B, Ph, Pw, C, dtype=qkv.dtype)
    idx = relative_position_index().reshape(WIN * WIN, WIN * WIN)
    bias = table.to(qkv.dtype)[idx].permute(2, 0, 1)                       # [heads, 49, 49]
    for wy in range(Ph // WIN):
        for wx in range(Pw // WIN):
            yy = sy[wy * WIN:(wy + 1) * WIN].repeat_interleave(WIN)       # token t = ty * 7 + tx of the window
            xx = sx[wx * WIN:(wx + 1) * WIN].repeat(WIN)
            lab = ly[wy * WIN:(wy + 1) * WIN].repeat_interleave(WIN) * 3 + lx[wx * WIN:(wx + 1) * WIN].repeat(WIN)
            tok = full[:, yy, xx].reshape(B, WIN * WIN, 3, heads, D).permute(2, 0, 3, 1, 4)
            q, k, v = tok[0] * D ** -0.5, tok[1], tok[2]
            s = q @ k.transpose(-1, -2) + bias
            if sh + sw > 0:
                s = s + (lab[:, None] != lab[None, :]).to(qkv.dtype) * -100.0
            o = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, WIN * WIN, C)
            out[:, yy, xx] = o
    return out[:, :H, :W].contiguous()


def layer_norm(x, w, b, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


def merge_gather(x):
    """[B, H, W, C] -> [B, ceil(H/2), ceil(W/2), 4C]: (x(0,0), x(1,0), x(0,1), x(1,1)) of every 2x2 cell, zeros past the edge."""
    B, H, W, C = x.shape
    xp = torch.zeros(B, H + H % 2, W + W % 2, C, dtype=x.dtype)
    xp[:, :H, :W] = x
    return torch.cat([xp[:, dy::2, dx::2] for dx in (0, 1) for dy in (0, 1)], dim=-1)


def merge_ln(x, w, b):
    return layer_norm(merge_gather(x), w, b)


def patch_merging(sd, p, x):
    return merge_ln(x, sd[p + "norm.weight"], sd[p + "norm.bias"]) @ sd[p + "reduction.weight"].t()


def attention(sd, p, x, heads, shift):
    qkv = x @ sd[p + "qkv.weight"].t() + sd[p + "qkv.bias"]
    o = attn_core(qkv, sd[p + "qkv.bias"], sd[p + "relative_position_bias_table"], heads, shift)
    return o @ sd[p + "proj.weight"].t() + sd[p + "proj.bias"]


def block(sd, p, x, heads, shift):
    x = x + attention(sd, p + "attn.", layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"]), heads, shift)
    h = layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"])
    h = F.gelu(h @ sd[p + "mlp.0.weight"].t() + sd[p + "mlp.0.bias"])
    return x + h @ sd[p + "mlp.3.weight"].t() + sd[p + "mlp.3.bias"]


def forward(sd, x, depths, num_heads):
    """x NCHW -> the four stage outputs as NCHW maps."""
    h = F.conv2d(x, sd["first_coonv.0.weight"], sd["first_coonv.0.bias"], stride=4).permute(0, 2, 3, 1)
    h = layer_norm(h, sd["first_coonv.2.weight"], sd["first_coonv.2.bias"])
    feats = []
    for st, (d, nh) in enumerate(zip(depths, num_heads)):
        for i in range(d):
            h = block(sd, f"features.{2 * st}.{i}.", h, nh, 0 if i % 2 == 0 else WIN // 2)
        feats.append(h.permute(0, 3, 1, 2).contiguous())
        if st < len(depths) - 1:
            h = patch_merging(sd, f"features.{2 * st + 1}.", h)
    return feats


# ------------------------------------------------------------------------------------------------ the cases' inputs
def attn_case_inputs(name, dtype=torch.float64):
    """x [B, H, W, C] and the hash-filled parameters of one attention module; proj is the identity without bias in the
    attention-alone cases, so that the module's output is the core's."""
    B, H, W, C, heads, shift = ATTN_CASES[name]
    p = f"{name}."
    sd = {p + "qkv.weight": fill_value(p + "qkv.weight", (3 * C, C), dtype),
          p + "qkv.bias": fill_value(p + "qkv.bias", (3 * C,), dtype),
          p + "relative_position_bias_table": fill_value(p + "relative_position_bias_table", ((2 * WIN - 1) ** 2, heads), dtype)}
    x = fill.hash_tensor((B, H, W, C), p + "x", 1.5, dtype)
    return x, sd


def attn_case_core(name, dtype=torch.float64):
    """(qkv, qkv_bias, table, heads, shift) of a case: the operands of the attention core."""
    _, _, _, _, heads, shift = ATTN_CASES[name]
    x, sd = attn_case_inputs(name, dtype)
    p = f"{name}."
    qkv = x @ sd[p + "qkv.weight"].t() + sd[p + "qkv.bias"]
    return qkv, sd[p + "qkv.bias"], sd[p + "relative_position_bias_table"], heads, shift


def merge_case_inputs(name, dtype=torch.float64):
    B, H, W, C = MERGE_CASES[name]
    p = f"{name}."
    sd = {p + "reduction.weight": fill_value(p + "reduction.weight", (2 * C, 4 * C), dtype),
          p + "norm.weight": fill_value(p + "norm.weight", (4 * C,), dtype),
          p + "norm.bias": fill_value(p + "norm.bias", (4 * C,), dtype)}
    return fill.hash_tensor((B, H, W, C), p + "x", 1.5, dtype) + 0.25, sd


def model_input(name, shape, dtype=torch.float64):
    return fill.hash_tensor(shape, f"swin.{name}.x", 1.0, dtype)


def load_golden():
    return np.load(GOLDEN)
