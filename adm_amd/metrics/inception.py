"""InceptionV3 feature extractor for FID / Inception score on the HIP hot path (csrc/inception.hip).

The network is the 2015-12-05 TensorFlow Inception graph as torch-fidelity ships it (the reference's
metrics/feature_extractor_inceptionv3.py): a TensorFlow-1 bilinear resize to 299x299, ``(v - 128) / 128``, 94 conv + BatchNorm(eval,
eps 1e-3) + ReLU units, 3x3 pools whose averages count in-image taps only, a max pool in the pool branch of Mixed_7c, and a
2048 -> 1008 fc.  The module tree and its 566 state-dict names are the reference's, so a local copy of torch-fidelity's
``weights-inception-2015-12-05`` file loads with ``strict=True``.  **No weights ship with this package and nothing is ever fetched:**
``from_file`` raises when the path does not exist.

The modules are parameter containers.  ``forward`` walks the table below: every unit is one ``adm_conv_rect_relu_fwd`` launch with
BatchNorm folded into weight and bias (in float64, once, when the weights are first used; the packed operands are cached because
the weights are frozen), and every branch writes its slice of the block's output buffer, so no concatenation pass exists.  The
kernels are the exact f32 MFMA whatever ``ADM_*`` compute mode the training path runs in.
"""
from __future__ import annotations

import os
from typing import Dict, List, Sequence, Tuple

import torch
import torch.nn as nn

from .. import hip

FEATURES = ("64", "192", "768", "2048", "logits_unbiased", "logits")
BN_EPS = 1e-3
INPUT_SIZE = 299


def pad32(c: int) -> int:
    return (c + 31) // 32 * 32


# ---------------------------------------------------------------------------------------------------- the network as a table
# A unit is (name, cin, cout, (kh, kw), stride, (pad_h, pad_w)).  A block is a list of branches (pool, chain, tails): ``pool`` is a
# pool mode applied to the block input first (or None), ``chain`` are units run in sequence, ``tails`` are units that each read the
# chain's result and write the next slice of the block output.  A branch without units writes its pooled input.
MAX_S2, MAX_S1, AVG_S1 = 0, 1, 2


def _u(name, cin, cout, k=1, s=1, p=0):
    k = (k, k) if isinstance(k, int) else k
    p = (p, p) if isinstance(p, int) else p
    return (name, cin, cout, k, s, p)


STEM = (_u("Conv2d_1a_3x3", 3, 32, 3, 2), _u("Conv2d_2a_3x3", 32, 32, 3), _u("Conv2d_2b_3x3", 32, 64, 3, 1, 1), MAX_S2,
        _u("Conv2d_3b_1x1", 64, 80), _u("Conv2d_4a_3x3", 80, 192, 3), MAX_S2)


def _block_a(cin, pool):
    return [(None, [], [_u("branch1x1", cin, 64)]),
            (None, [_u("branch5x5_1", cin, 48)], [_u("branch5x5_2", 48, 64, 5, 1, 2)]),
            (None, [_u("branch3x3dbl_1", cin, 64), _u("branch3x3dbl_2", 64, 96, 3, 1, 1)], [_u("branch3x3dbl_3", 96, 96, 3, 1, 1)]),
            (AVG_S1, [], [_u("branch_pool", cin, pool)])]


def _block_b(cin):
    return [(None, [], [_u("branch3x3", cin, 384, 3, 2)]),
            (None, [_u("branch3x3dbl_1", cin, 64), _u("branch3x3dbl_2", 64, 96, 3, 1, 1)], [_u("branch3x3dbl_3", 96, 96, 3, 2)]),
            (MAX_S2, [], [])]


def _block_c(cin, c7):
    row, col = dict(k=(1, 7), p=(0, 3)), dict(k=(7, 1), p=(3, 0))
    return [(None, [], [_u("branch1x1", cin, 192)]),
            (None, [_u("branch7x7_1", cin, c7), _u("branch7x7_2", c7, c7, **row)], [_u("branch7x7_3", c7, 192, **col)]),
            (None, [_u("branch7x7dbl_1", cin, c7), _u("branch7x7dbl_2", c7, c7, **col), _u("branch7x7dbl_3", c7, c7, **row),
                    _u("branch7x7dbl_4", c7, c7, **col)], [_u("branch7x7dbl_5", c7, 192, **row)]),
            (AVG_S1, [], [_u("branch_pool", cin, 192)])]


def _block_d(cin):
    return [(None, [_u("branch3x3_1", cin, 192)], [_u("branch3x3_2", 192, 320, 3, 2)]),
            (None, [_u("branch7x7x3_1", cin, 192), _u("branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)),
                    _u("branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))], [_u("branch7x7x3_4", 192, 192, 3, 2)]),
            (MAX_S2, [], [])]


def _block_e(cin, pool):
    row, col = dict(k=(1, 3), p=(0, 1)), dict(k=(3, 1), p=(1, 0))
    return [(None, [], [_u("branch1x1", cin, 320)]),
            (None, [_u("branch3x3_1", cin, 384)], [_u("branch3x3_2a", 384, 384, **row), _u("branch3x3_2b", 384, 384, **col)]),
            (None, [_u("branch3x3dbl_1", cin, 448), _u("branch3x3dbl_2", 448, 384, 3, 1, 1)],
             [_u("branch3x3dbl_3a", 384, 384, **row), _u("branch3x3dbl_3b", 384, 384, **col)]),
            (pool, [], [_u("branch_pool", cin, 192)])]


# (name, branches, the feature tapped after the block or None); Mixed_7c's pool branch is a MAX pool in this graph
BLOCKS = (("Mixed_5b", _block_a(192, 32), None), ("Mixed_5c", _block_a(256, 64), None), ("Mixed_5d", _block_a(288, 64), None),
          ("Mixed_6a", _block_b(288), None), ("Mixed_6b", _block_c(768, 128), None), ("Mixed_6c", _block_c(768, 160), None),
          ("Mixed_6d", _block_c(768, 160), None), ("Mixed_6e", _block_c(768, 192), "768"),
          ("Mixed_7a", _block_d(768), None), ("Mixed_7b", _block_e(1280, AVG_S1), None), ("Mixed_7c", _block_e(2048, MAX_S1), None))


def block_units(branches):
    return [u for _, chain, tails in branches for u in list(chain) + list(tails)]


def all_units() -> List[Tuple[str, tuple]]:
    """(dotted module path, unit) for the 94 conv + BatchNorm units, in forward order."""
    out = [(u[0], u) for u in STEM if not isinstance(u, int)]
    for name, branches, _ in BLOCKS:
        out += [(f"{name}.{u[0]}", u) for u in block_units(branches)]
    return out


def state_dict_names() -> List[str]:
    names = []
    for path, _ in all_units():
        names += [f"{path}.conv.weight"] + [f"{path}.bn.{leaf}" for leaf in ("weight", "bias", "running_mean", "running_var",
                                                                              "num_batches_tracked")]
    return names + ["fc.weight", "fc.bias"]


def state_dict_shapes() -> Dict[str, Tuple[int, ...]]:
    shapes = {}
    for path, (_, cin, cout, k, _, _) in all_units():
        shapes[f"{path}.conv.weight"] = (cout, cin, k[0], k[1])
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{path}.bn.{leaf}"] = (cout,)
        shapes[f"{path}.bn.num_batches_tracked"] = ()
    shapes["fc.weight"], shapes["fc.bias"] = (1008, 2048), (1008,)
    return shapes


# ---------------------------------------------------------------------------------------------------- host arithmetic
def fold_bn(w, gamma, beta, mean, var, eps: float = BN_EPS):
    """conv (no bias) followed by eval-mode BatchNorm as one conv: float64 ``(w * s[:, None, None, None], beta - mean * s)`` with
    ``s = gamma / sqrt(var + eps)``."""
    w, gamma, beta, mean, var = (t.detach().double().cpu() for t in (w, gamma, beta, mean, var))
    s = gamma / torch.sqrt(var + eps)
    return w * s[:, None, None, None], beta - mean * s


def pack_rect(w64: torch.Tensor, b64, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """[cout][cin][kh][kw] float64 -> the kernel's operand [pad32(cout)][kh*kw*pad32(cin)] (k = (dy*kw + dx)*cin_p + c) and bias
    [pad32(cout)] in float32; padded rows and channels are zero."""
    co, ci, kh, kw = w64.shape
    wp = torch.zeros(pad32(co), kh, kw, pad32(ci), dtype=torch.float64)
    wp[:co, :, :, :ci] = w64.permute(0, 2, 3, 1)
    bp = torch.zeros(pad32(co), dtype=torch.float64)
    if b64 is not None:
        bp[:co] = b64
    return wp.reshape(pad32(co), -1).float().contiguous().to(device), bp.float().to(device)


# ---------------------------------------------------------------------------------------------------- kernel wrappers
def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def conv_rect(x: torch.Tensor, wp: torch.Tensor, bias, k, stride=1, pad=(0, 0), out=None, yoff=0, cin=None, relu=True, tile=-1):
    """relu(conv(x) + bias) of NHWC f32 ``x`` (its first ``cin`` channels; default all) with a packed operand of ``pack_rect``;
    written to ``out[..., yoff:yoff + wp.shape[0]]`` (a fresh tensor when ``out`` is None)."""
    hip.require_cuda(x, "conv_rect input")
    B, H, W, ldx = x.shape
    cin = ldx if cin is None else cin
    N = wp.shape[0]
    Ho, Wo = conv_out(H, k[0], stride, pad[0]), conv_out(W, k[1], stride, pad[1])
    if wp.shape[1] != k[0] * k[1] * cin:
        raise ValueError(f"packed weight has K = {wp.shape[1]}, the call implies {k[0] * k[1] * cin}")
    if out is None:
        out = torch.empty(B, Ho, Wo, N, device=x.device, dtype=torch.float32)
    if tuple(out.shape[:3]) != (B, Ho, Wo) or not out.is_contiguous() or not x.is_contiguous():
        raise ValueError(f"conv_rect: output {tuple(out.shape)} does not fit [{B}, {Ho}, {Wo}, *] or a tensor is not contiguous")
    hip.call("adm_conv_rect_relu_fwd", hip.ptr(x), hip.ptr(wp), hip.ptr(bias), hip.ptr(out), B, H, W, cin, ldx, N, out.shape[3],
             yoff, k[0], k[1], stride, pad[0], pad[1], 1 if relu else 0, tile)
    return out


def pool3x3(x: torch.Tensor, mode: int, out=None, yoff=0):
    hip.require_cuda(x, "pool3x3 input")
    B, H, W, C = x.shape
    Ho, Wo = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if mode == MAX_S2 else (H, W)
    if out is None:
        out = torch.empty(B, Ho, Wo, C, device=x.device, dtype=torch.float32)
    if tuple(out.shape[:3]) != (B, Ho, Wo) or not out.is_contiguous() or not x.is_contiguous():
        raise ValueError(f"pool3x3: output {tuple(out.shape)} does not fit [{B}, {Ho}, {Wo}, *] or a tensor is not contiguous")
    hip.call("adm_pool3x3_fwd", hip.ptr(x), hip.ptr(out), B, H, W, C, C, out.shape[3], yoff, mode)
    return out


def global_avgpool(x: torch.Tensor, C=None):
    hip.require_cuda(x, "global_avgpool input")
    B, H, W, ldx = x.shape
    C = ldx if C is None else C
    y = torch.empty(B, C, device=x.device, dtype=torch.float32)
    hip.call("adm_global_avgpool_fwd", hip.ptr(x.contiguous()), hip.ptr(y), B, H, W, C, ldx)
    return y


def tf1_resize_norm(img: torch.Tensor):
    """uint8 [B,3,H,W] -> [B,299,299,32] f32: the TensorFlow-1 resize and ``(v - 128) / 128``, channels 3..31 zero."""
    hip.require_cuda(img, "image batch")
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f"expected a uint8 [B,3,H,W] batch, got {img.dtype} {tuple(img.shape)}")
    img = img.contiguous()
    B, _, H, W = img.shape
    y = torch.empty(B, INPUT_SIZE, INPUT_SIZE, 32, device=img.device, dtype=torch.float32)
    hip.call("adm_tf1_resize_norm_u8", hip.ptr(img), hip.ptr(y), B, H, W)
    return y


# ---------------------------------------------------------------------------------------------------- the module
class _ConvBN(nn.Module):
    """Holder of one unit's parameters under the reference's names ``conv.weight`` and ``bn.*``."""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv = nn.Module()
        self.conv.weight = nn.Parameter(torch.zeros(cout, cin, k[0], k[1]), requires_grad=False)
        self.bn = nn.Module()
        self.bn.weight = nn.Parameter(torch.ones(cout), requires_grad=False)
        self.bn.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)
        self.bn.register_buffer("running_mean", torch.zeros(cout))
        self.bn.register_buffer("running_var", torch.ones(cout))
        self.bn.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class FeatureExtractorInceptionV3(nn.Module):
    def __init__(self, features_list: Sequence[str] = ("2048",)):
        super().__init__()
        features_list = list(features_list)
        bad = [f for f in features_list if f not in FEATURES]
        if bad or not features_list or len(set(features_list)) != len(features_list):
            raise ValueError(f"features_list {features_list}: expected distinct names out of {FEATURES}")
        self.features_list = features_list
        for u in STEM:
            if not isinstance(u, int):
                self.add_module(u[0], _ConvBN(u[1], u[2], u[3]))
        for name, branches, _ in BLOCKS:
            blk = nn.Module()
            for u in block_units(branches):
                blk.add_module(u[0], _ConvBN(u[1], u[2], u[3]))
            self.add_module(name, blk)
        self.fc = nn.Module()
        self.fc.weight = nn.Parameter(torch.zeros(1008, 2048), requires_grad=False)
        self.fc.bias = nn.Parameter(torch.zeros(1008), requires_grad=False)
        self._packed = None
        self.eval()

    @staticmethod
    def get_provided_features_list():
        return FEATURES

    def train(self, mode: bool = True):
        return super().train(False)

    def load_state_dict(self, *a, **kw):
        self._packed = None
        return super().load_state_dict(*a, **kw)

    def _apply(self, fn, *a, **kw):
        self._packed = None
        return super()._apply(fn, *a, **kw)

    @classmethod
    def from_file(cls, path: str, features_list: Sequence[str] = ("2048",)) -> "FeatureExtractorInceptionV3":
        """From a local state dict in the reference's layout.  A missing file raises: there is no download."""
        if not path or not os.path.isfile(path):
            raise FileNotFoundError(f"InceptionV3 weights file {path!r} does not exist; copy torch-fidelity's "
                                    "weights-inception-2015-12-05 state dict to this machine (nothing is fetched)")
        sd = torch.load(path, map_location="cpu", weights_only=True)
        m = cls(features_list)
        m.load_state_dict(sd, strict=True)
        return m

    # ------------------------------------------------------------------ packed operands
    def _operands(self, device):
        if self._packed is None or self._packed[0] != device:
            ops = {}
            for path, u in all_units():
                m = self.get_submodule(path)
                w64, b64 = fold_bn(m.conv.weight, m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var)
                ops[path] = pack_rect(w64, b64, device)
            fw = self.fc.weight.detach().double().cpu()[:, :, None, None]
            ops["fc"] = pack_rect(fw, self.fc.bias.detach().double().cpu(), device)
            self._packed = (device, ops)
        return self._packed[1]

    def _unit(self, ops, path, u, x, out=None, yoff=0):
        wp, b = ops[path]
        return conv_rect(x, wp, b, u[3], u[4], u[5], out=out, yoff=yoff, cin=pad32(u[1]))

    def _block(self, ops, name, branches, x):
        B, H, W, _ = x.shape
        width, Ho, Wo = 0, H, W
        for pool, chain, tails in branches:
            width += sum(pad32(t[2]) for t in tails) if tails else x.shape[3]
            last = tails[0] if tails else None
            if (last is not None and last[4] == 2) or (last is None and pool == MAX_S2):
                Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        out = torch.empty(B, Ho, Wo, width, device=x.device, dtype=torch.float32)
        off = 0
        for pool, chain, tails in branches:
            if not tails:
                pool3x3(x, pool, out=out, yoff=off)
                off += x.shape[3]
                continue
            h = x if pool is None else pool3x3(x, pool)
            for u in chain:
                h = self._unit(ops, f"{name}.{u[0]}", u, h)
            for u in tails:
                self._unit(ops, f"{name}.{u[0]}", u, h, out=out, yoff=off)
                off += pad32(u[2])
        return out

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, x: torch.Tensor, taps: dict = None):
        """uint8 [B,3,H,W] on the GPU -> tuple of [B, d] f32 in the order of ``features_list``; returns as soon as the last requested
        feature exists.  ``taps`` (a dict) receives the spatial mean of every Mixed_* output, for locating a discrepancy."""
        if not torch.is_tensor(x) or x.dtype != torch.uint8:
            raise ValueError("expecting a uint8 image batch [B,3,H,W]")
        ops = self._operands(x.device)
        features, remaining = {}, list(self.features_list)

        def done(name, value):
            if name in remaining:
                features[name] = value() if callable(value) else value
                remaining.remove(name)
            return not remaining

        def result():
            return tuple(features[f] for f in self.features_list)

        h = tf1_resize_norm(x)
        for i, u in enumerate(STEM):
            h = pool3x3(h, u) if isinstance(u, int) else self._unit(ops, u[0], u, h)
            if i == 3 and done("64", lambda: global_avgpool(h)):
                return result()
        if done("192", lambda: global_avgpool(h)):
            return result()
        for name, branches, tap in BLOCKS:
            h = self._block(ops, name, branches, h)
            if taps is not None:
                taps[name] = global_avgpool(h)
            if tap is not None and done(tap, lambda: global_avgpool(h)):
                return result()
        pooled = global_avgpool(h)
        if done("2048", pooled):
            return result()
        wp, b = ops["fc"]
        p4 = pooled.view(pooled.shape[0], 1, 1, 2048)
        if "logits_unbiased" in remaining:
            unbiased = conv_rect(p4, wp, None, (1, 1), relu=False).view(-1, wp.shape[0])[:, :1008].contiguous()
            if done("logits_unbiased", unbiased):
                return result()
            logits = unbiased + self.fc.bias.to(unbiased.device)[None]
        else:
            logits = conv_rect(p4, wp, b, (1, 1), relu=False).view(-1, wp.shape[0])[:, :1008].contiguous()
        features["logits"] = logits
        return result()
