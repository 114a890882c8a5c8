"""Training-side companion of tests/swin_ref.py (TEST INFRASTRUCTURE ONLY): the Swin block with stochastic depth as per-sample
row scales, the p_k schedule, the loss the gradient tests differentiate and fp64 autograd over the restatement.

Restated from the reference's unet/swin_transformer.py: SwinTransformerBlock.forward :302-305 with
``StochasticDepth(sd_prob, "row")`` (:292) around both branches, and sd_prob = p * k / (n_blocks - 1) over the running block
index (:371-393).  torchvision's StochasticDepth in "row" mode, as the reference uses it: in training and with p > 0 the branch
of sample b is multiplied by keep_b / (1 - p), keep_b ~ Bernoulli(1 - p); otherwise it is the identity.  Here the draws are an
argument (``keep`` [n_blocks, 2, B] of 0 / 1: block, branch (attention, MLP), sample).

tests/golden/g20_swin_train.npz (tools/make_golden_swin_train.py) holds gradients the reference's own classes gave in float64
and train mode, sampled by ``sample_grad``.
"""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import swin_ref as R
from oracle import fill

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_swin_train.npz")

# the injected draws of the SMALL model (8 blocks, 2 samples): [block][branch][sample].  Block 0 has p_0 = 0 (its row is unused);
# samples are dropped in early, middle and late blocks, in either branch, the last block included.
KEEP_SMALL = torch.tensor([[[1, 1], [1, 1]],
                           [[1, 1], [1, 0]],
                           [[1, 0], [1, 1]],
                           [[1, 1], [1, 1]],
                           [[0, 1], [1, 1]],
                           [[1, 1], [0, 1]],
                           [[1, 1], [1, 0]],
                           [[0, 1], [1, 1]]], dtype=torch.float64)


def sample_grad(a):
    """What the golden file keeps of a gradient: every 15th element of swin_ref.sample (at most ~274 values)."""
    return R.sample(a)[::15]


def sd_probs(depths, p):
    """p_k = p * k / (n_blocks - 1) for the running block index k (reference :379)."""
    n = sum(depths)
    return [p * float(k) / (n - 1) for k in range(n)]


def scales_from_keep(keep, probs):
    """[n_blocks, 2, B] row scales keep / (1 - p_k); None entries where p_k == 0 (the branch joins unscaled)."""
    return [None if p == 0.0 else keep[k].to(torch.float64) / (1.0 - p) for k, p in enumerate(probs)]


def block(sd, p, x, heads, shift, scales=None):
    a = R.attention(sd, p + "attn.", R.layer_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"]), heads, shift)
    x = x + (a if scales is None else a * scales[0].to(a.dtype).view(-1, 1, 1, 1))
    h = R.layer_norm(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"])
    h = F.gelu(h @ sd[p + "mlp.0.weight"].t() + sd[p + "mlp.0.bias"])
    h = h @ sd[p + "mlp.3.weight"].t() + sd[p + "mlp.3.bias"]
    return x + (h if scales is None else h * scales[1].to(h.dtype).view(-1, 1, 1, 1))


def forward(sd, x, depths, num_heads, scales=None):
    """swin_ref.forward with the per-block row scales of ``scales_from_keep`` (None: every branch joins unscaled)."""
    h = F.conv2d(x, sd["first_coonv.0.weight"], sd["first_coonv.0.bias"], stride=4).permute(0, 2, 3, 1)
    h = R.layer_norm(h, sd["first_coonv.2.weight"], sd["first_coonv.2.bias"])
    feats, k = [], 0
    for st, (d, nh) in enumerate(zip(depths, num_heads)):
        for i in range(d):
            h = block(sd, f"features.{2 * st}.{i}.", h, nh, 0 if i % 2 == 0 else R.WIN // 2, None if scales is None else scales[k])
            k += 1
        feats.append(h.permute(0, 3, 1, 2).contiguous())
        if st < len(depths) - 1:
            h = R.patch_merging(sd, f"features.{2 * st + 1}.", h)
    return feats


# ------------------------------------------------------------------------------------------------ losses and gradients
def weight_like(t, tag, dtype=torch.float64):
    """The hash-filled cotangent of a tensor: loss = sum(t * weight_like(t))."""
    return fill.hash_tensor(tuple(t.shape), f"swin_train.{tag}", 1.0, dtype)


def model_loss(feats, tag):
    return sum((f * weight_like(f, f"{tag}.stage{i}", f.dtype)).sum() for i, f in enumerate(feats))


def trainable_names(sd):
    """The parameters forward uses: everything floating point but norm.* / head.* (and not the index buffers)."""
    return [k for k, v in sd.items() if v.is_floating_point() and not k.startswith(("norm.", "head."))]


def model_grads(cfg, shape, name, tag, keep=None, p=0.0):
    """fp64 autograd over the restatement: {parameter name: gradient} plus "x" for the input, loss = model_loss(feats, tag)."""
    sd = R.filled_state_dict(**cfg)
    names = trainable_names(sd)
    for k in names:
        sd[k] = sd[k].clone().requires_grad_(True)
    x = R.model_input(name, shape).requires_grad_(True)
    scales = None if keep is None else scales_from_keep(keep, sd_probs(cfg["depths"], p))
    feats = forward(sd, x, cfg["depths"], cfg["num_heads"], scales)
    gs = torch.autograd.grad(model_loss(feats, tag), [sd[k] for k in names] + [x])
    out = OrderedDict(zip(names, gs[:-1]))
    out["x"] = gs[-1]
    return out


def attn_core_grads(name):
    """fp64 gradients of the attention core alone: (d_qkv, d_qkv_bias, d_table, d_out) with d_out hash-filled.  The bias here is
    the core's own operand: its gradient is the padding tokens' share only."""
    qkv, qb, table, heads, shift = R.attn_case_core(name)
    qkv, qb, table = (t.detach().clone().requires_grad_(True) for t in (qkv, qb, table))
    out = R.attn_core(qkv, qb, table, heads, shift)
    d_out = weight_like(out, f"attn.{name}.d_out")
    return torch.autograd.grad((out * d_out).sum(), [qkv, qb, table]) + (d_out,)


def attn_module_grads(name):
    """fp64 gradients of the attention MODULE of a case (qkv Linear + core, identity proj), as the golden file holds them:
    dx, dqkv_w, dqkv_b (both shares), dtable."""
    _, _, _, _, heads, shift = R.ATTN_CASES[name]
    x, sd = R.attn_case_inputs(name)
    p = f"{name}."
    x = x.clone().requires_grad_(True)
    w, b, t = (sd[p + k].clone().requires_grad_(True) for k in ("qkv.weight", "qkv.bias", "relative_position_bias_table"))
    out = R.attn_core(x @ w.t() + b, b, t, heads, shift)
    gs = torch.autograd.grad((out * weight_like(out, f"attn.{name}.d_out")).sum(), [x, w, b, t])
    return OrderedDict(zip(("dx", "dqkv_w", "dqkv_b", "dtable"), gs))


def merge_grads(name):
    """fp64 gradients of PatchMerging on a case: dx, dnorm_w, dnorm_b, dred_w."""
    x, sd = R.merge_case_inputs(name)
    x = x.clone().requires_grad_(True)
    sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    out = R.patch_merging(sd, name + ".", x)
    gs = torch.autograd.grad((out * weight_like(out, f"merge.{name}.d_out")).sum(),
                             [x, sd[name + ".norm.weight"], sd[name + ".norm.bias"], sd[name + ".reduction.weight"]])
    return OrderedDict(zip(("dx", "dnorm_w", "dnorm_b", "dred_w"), gs))


def load_golden():
    return np.load(GOLDEN)
