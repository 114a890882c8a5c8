"""The single-channel Swin condition encoder for the tests (TEST INFRASTRUCTURE ONLY): tests/swin_ref.py and
tests/swin_train_ref.py reused unchanged, with the one thing the reference's unet/swin_transformer_for_sci.py changes in the module
-- the patch-embedding conv takes ONE input channel (:365) -- restated as the stem's shape.  (Its other change, the mean of the
ImageNet stem over the input channels at load time, :458-459, is the loader's and is tested there.)

Also the cases of the fused stem kernel (adm_patch_embed_ln_fwd / _bwd) and of tests/golden/g25_swin_sci.npz
(tools/make_golden_swin_sci.py): what the reference's own classes gave in float64, sampled by ``swin_ref.sample`` /
``swin_train_ref.sample_grad``.
"""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import swin_ref as R
import swin_train_ref as T
from oracle import fill

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_swin_sci.npz")

# the stem alone, forward: name -> (B, H, W, E)
STEM_CASES = OrderedDict([
    ("s30x44", (2, 30, 44, 32)),        # ragged on both axes: 7 x 11 tokens, more than one workgroup with a partial last one
    ("s64x64", (1, 64, 64, 128)),
    ("s8x4", (3, 8, 4, 128)),           # a single token column
    ("s4x4", (1, 4, 4, 32)),            # one token
])
STEM_CONTENTS = ("plain", "offset", "zero")        # hash-filled rows, the same on a common offset of +300, an all-zero image
# the stem alone, backward (fp64 autograd in the test, not stored): 792 and 77 tokens, multiples of no block size
STEM_BWD_CASES = OrderedDict([("g72x88", (2, 72, 88, 32)), ("g30x44", (1, 30, 44, 128))])
SMALL_INPUT = (2, 1, 72, 88)
SWIN_B_INPUT = (1, 1, 64, 64)
STEM_NAMES = ("first_coonv.0.weight", "first_coonv.0.bias", "first_coonv.2.weight", "first_coonv.2.bias")
TRAIN_TAGS = (("sci.sd0", 0.0, None), ("sci.sd5", 0.5, T.KEEP_SMALL))


def stem_params(E, dtype=torch.float64):
    """{first_coonv.*: tensor} of a stem of width E, by swin_ref's fill rule (the tag carries E)."""
    shapes = {"first_coonv.0.weight": (E, 1, 4, 4), "first_coonv.0.bias": (E,), "first_coonv.2.weight": (E,), "first_coonv.2.bias": (E,)}
    return OrderedDict((k, R.fill_value(f"sci{E}.{k}", s, dtype)) for k, s in shapes.items())


def stem_input(name, content, dtype=torch.float64, cases=STEM_CASES):
    B, H, W, _ = cases[name]
    if content == "zero":
        return torch.zeros(B, 1, H, W, dtype=dtype)
    x = fill.hash_tensor((B, 1, H, W), f"swin_sci.{name}.x", 1.0, dtype)
    return x + 300.0 if content == "offset" else x


def stem(sd, x, eps=1e-5):
    """Conv2d(1, E, 4, 4) -> NHWC -> LayerNorm(E): [B, 1, H, W] -> [B, H // 4, W // 4, E]."""
    h = F.conv2d(x, sd["first_coonv.0.weight"], sd["first_coonv.0.bias"], stride=4).permute(0, 2, 3, 1)
    return R.layer_norm(h, sd["first_coonv.2.weight"], sd["first_coonv.2.bias"], eps)


def param_shapes(embed_dim, depths, num_heads, num_classes=1000):
    s = R.param_shapes(embed_dim, depths, num_heads, num_classes)
    s["first_coonv.0.weight"] = (embed_dim, 1, 4, 4)
    return s


def filled_state_dict(embed_dim, depths, num_heads, num_classes=1000, dtype=torch.float64):
    """swin_ref.filled_state_dict with the one-channel stem weight (its own fill: fan-in 16)."""
    return OrderedDict((k, R.fill_value(k, s, dtype)) for k, s in param_shapes(embed_dim, depths, num_heads, num_classes).items())


def model_input(name, shape, dtype=torch.float64):
    return R.model_input(f"sci.{name}", shape, dtype)


def forward(sd, x, depths, num_heads):
    """swin_ref.forward: its stem is F.conv2d with the state dict's weight, so the one-channel weight is all it takes."""
    assert x.shape[1] == 1 and sd["first_coonv.0.weight"].shape[1] == 1
    return R.forward(sd, x, depths, num_heads)


def stem_grads(cfg, shape, name, tag, keep=None, p=0.0):
    """swin_train_ref.model_grads over the one-channel state dict, reduced to {first_coonv.*: gradient} (the input takes none)."""
    sd = filled_state_dict(**cfg)
    names = T.trainable_names(sd)
    for k in names:
        sd[k] = sd[k].clone().requires_grad_(True)
    x = model_input(name, shape)
    scales = None if keep is None else T.scales_from_keep(keep, T.sd_probs(cfg["depths"], p))
    feats = T.forward(sd, x, cfg["depths"], cfg["num_heads"], scales)
    gs = torch.autograd.grad(T.model_loss(feats, tag), [sd[k] for k in STEM_NAMES])
    return OrderedDict(zip(STEM_NAMES, gs))


def load_golden():
    return np.load(GOLDEN)
