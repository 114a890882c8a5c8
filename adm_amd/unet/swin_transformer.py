"""MI355X-native Swin condition encoder behind the reference's module API: the ``init_conv_mask`` of the conditional denoisers
(/root/reference/unet/swin_transformer.py, built at cond_unet_sd.py:637-650 and cond_unet.py of the reference as ``swin_b``).

Same constructor keywords, same module tree and therefore the same ``state_dict()`` names and shapes (torch.nn
modules are PARAMETER HOLDERS: ``first_coonv`` (sic), ``features.{0..6}``, and the never-used ``norm`` / ``head`` so that a strict
load of a reference checkpoint passes).  ``forward(x)`` takes the NCHW condition image and returns the four stage outputs as
NCHW maps (E, 2E, 4E, 8E channels at 1/4 ... 1/32), computed on HIP kernels: the fused shifted-window attention, LayerNorm and
PatchMerging kernels of csrc/swin.hip around the GEMM / GELU / residual kernels of ``adm_amd.ops`` -- there is no PyTorch fallback.

FROZEN BY DEFAULT, TRAINING IS OPT-IN.  Every parameter is created with ``requires_grad=False`` (the reference's own
``fix_bb: True`` state) and the forward runs without grad and with eval semantics, until ``enable_training()`` is called:
that sets ``requires_grad`` on every parameter ``forward`` uses (``norm.*`` / ``head.*`` stay frozen: they are never used, the
reference leaves their ``.grad`` at None), makes ``forward`` run with grad through the HIP backward kernels of
``adm_amd.ops_swin``, and switches stochastic depth on in ``.train()`` mode: torchvision's ``StochasticDepth(p_k, "row")`` around
both branches of block k, p_k = p * k / (n_blocks - 1) (reference :292,303-304,379), restated in ``ops_swin.row_scale_add``.
Nothing is ever fetched: the weights come from the checkpoint of the conditional model.  Attention / output dropout (0.0 in
every config), EfficientNet-B7 and ResNet-101 are not built.

``in_chans=1`` is the single-channel variant (/root/reference/unet/swin_transformer_for_sci.py, ``single_channel_cond: True``): the
patch-embedding conv takes one channel (reference :365) and runs fused with its LayerNorm in ``ops_swin.patch_embed_ln``;
``load_encoder_weights`` averages a 3-channel ImageNet stem over its input channels (reference :458-459).  Everything else is shared.

Reference lines restated: PatchMerging :51-68, shifted_window_attention :71-168, ShiftedWindowAttention :174-248,
SwinTransformerBlock :251-305, SwinTransformer :308-425.
"""
from __future__ import annotations

import warnings
from typing import List, Optional

import torch
import torch.nn as nn

from .. import hip, ops
from .. import ops_cond as oc
from .. import ops_swin as osw

__all__ = ["SwinTransformer", "swin_b"]


def _linear(x, lin: nn.Linear, residual=None):
    """nn.Linear over the last axis of an NHWC tensor (+ residual in the GEMM's epilogue)."""
    lead = x.shape[:-1]
    r = None if residual is None else residual.reshape(-1, residual.shape[-1])
    return ops.linear(x.reshape(-1, x.shape[-1]), lin.weight, lin.bias, r).reshape(*lead, lin.out_features)


class PatchMerging(nn.Module):
    def __init__(self, dim: int, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)

    def forward(self, x):
        return _linear(osw.merge_layer_norm(x, self.norm.weight, self.norm.bias, self.norm.eps), self.reduction)


class ShiftedWindowAttention(nn.Module):
    def __init__(self, dim: int, window_size: List[int], shift_size: List[int], num_heads: int, qkv_bias: bool = True,
                 proj_bias: bool = True, attention_dropout: float = 0.0, dropout: float = 0.0):
        super().__init__()
        if (list(window_size) != [osw.WINDOW, osw.WINDOW] or len(shift_size) != 2 or dim != num_heads * osw.HEAD_DIM
                or not (qkv_bias and proj_bias)):
            raise NotImplementedError("the window attention kernel is specialised to 7x7 windows and heads of 32 channels with "
                                      "biases (Swin-T / -S / -B)")
        self.window_size, self.shift_size, self.num_heads = list(window_size), list(shift_size), num_heads
        self.qkv = nn.Linear(dim, dim * 3)
        self.proj = nn.Linear(dim, dim)
        self.relative_position_bias_table = nn.Parameter(torch.empty((2 * osw.WINDOW - 1) ** 2, num_heads))   # values: _init_weights
        self.register_buffer("relative_position_index", osw.relative_position_index())

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        # the kernel evaluates the index formula instead of reading this buffer: a checkpoint that holds another one is refused
        if not torch.equal(self.relative_position_index.cpu(), osw.relative_position_index()):
            raise RuntimeError(f"{prefix}relative_position_index of the checkpoint is not (dy + 6) * 13 + (dx + 6), the index the "
                               "window attention kernel computes")

    def forward(self, x, residual=None):
        """x [B, H, W, C] (already normalised); returns proj(attention) + residual.  The shift is switched off per axis, per
        call, inside the kernel (the reference writes it into the module, which makes it sticky across shapes)."""
        qkv = _linear(x, self.qkv)
        o = osw.window_attention(qkv, self.qkv.bias, self.relative_position_bias_table, self.num_heads, tuple(self.shift_size))
        return _linear(o, self.proj, residual)


class MLP(nn.Sequential):
    """torchvision.ops.misc.MLP's layout for one hidden layer: Linear, GELU, Dropout, Linear, Dropout (keys 0 and 3)."""

    def __init__(self, dim: int, hidden: int, dropout: float = 0.0):
        super().__init__(nn.Linear(dim, hidden), nn.GELU(), nn.Dropout(dropout), nn.Linear(hidden, dim), nn.Dropout(dropout))

    def forward(self, x, residual=None):
        return _linear(oc.gelu(_linear(x, self[0])), self[3], residual)


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim: int, num_heads: int, window_size: List[int], shift_size: List[int], mlp_ratio: float = 4.0,
                 dropout: float = 0.0, attention_dropout: float = 0.0, stochastic_depth_prob: float = 0.0,
                 norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = ShiftedWindowAttention(dim, window_size, shift_size, num_heads, attention_dropout=attention_dropout,
                                           dropout=dropout)
        self.norm2 = norm_layer(dim)
        self.mlp = MLP(dim, int(dim * mlp_ratio), dropout)
        self.sd_prob = 0.0          # set by SwinTransformer.enable_training(); the constructor's value is kept there

    def forward(self, x, scales=None):
        """scales: None (both branches join through the GEMM's fused residual) or the two [B] row scales keep / (1 - p) of
        stochastic depth, attention branch first."""
        h = osw.layer_norm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        x = self.attn(h, residual=x) if scales is None else osw.row_scale_add(x, self.attn(h), scales[0])
        h = osw.layer_norm(x, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        return self.mlp(h, residual=x) if scales is None else osw.row_scale_add(x, self.mlp(h), scales[1])


class SwinTransformer(nn.Module):
    def __init__(self, patch_size: List[int], embed_dim: int, depths: List[int], num_heads: List[int], window_size: List[int],
                 mlp_ratio: float = 4.0, dropout: float = 0.0, attention_dropout: float = 0.0, stochastic_depth_prob: float = 0.0,
                 num_classes: int = 1000, norm_layer=None, block=None, fix_bb: bool = True, in_chans: int = 3):
        super().__init__()
        if in_chans not in (1, 3):
            raise NotImplementedError(f"the condition encoder takes 3-channel images or, as the single-channel variant, 1-channel ones; "
                                      f"in_chans={in_chans} is not built")
        self.in_chans = int(in_chans)
        if list(patch_size) != [4, 4] or embed_dim % 32 or len(depths) != 4 or len(num_heads) != 4:
            raise NotImplementedError("4x4 patches, an embedding width that is a multiple of 32 and four stages (every reference "
                                      "config) are what is built")
        if norm_layer is not None or block is not None:
            raise NotImplementedError("custom norm_layer / block classes are not supported")
        norm_layer = lambda d: nn.LayerNorm(d, eps=1e-5)
        self.num_classes, self.fix_bb = num_classes, fix_bb
        self.stochastic_depth_prob = float(stochastic_depth_prob)      # used only after enable_training()
        self.trainable = False
        self._warned = False
        self.first_coonv = nn.Sequential(nn.Conv2d(self.in_chans, embed_dim, kernel_size=4, stride=4), nn.Identity(), norm_layer(embed_dim))
        layers: List[nn.Module] = []
        for i_stage in range(len(depths)):
            dim = embed_dim * 2 ** i_stage
            layers.append(nn.Sequential(*[
                SwinTransformerBlock(dim, num_heads[i_stage], window_size=list(window_size),
                                     shift_size=[(i_layer & 1) * (window_size[0] // 2), (i_layer & 1) * (window_size[1] // 2)],
                                     mlp_ratio=mlp_ratio, dropout=dropout, attention_dropout=attention_dropout, norm_layer=norm_layer)
                for i_layer in range(depths[i_stage])]))
            if i_stage < len(depths) - 1:
                layers.append(PatchMerging(dim, norm_layer))
        self.features = nn.ModuleList(layers)
        num_features = embed_dim * 2 ** (len(depths) - 1)
        self.norm = norm_layer(num_features)              # norm / head: never used by forward (reference :419-424), kept as holders
        self.head = nn.Linear(num_features, num_classes)
        self._init_weights()
        for p in self.parameters():                        # frozen until enable_training()
            p.requires_grad_(False)

    def _init_weights(self):
        """Placeholder values until a checkpoint is loaded (every real use loads one): matrices and the bias tables small
        truncated-normal, vectors of the Linears zero; the stem conv and the LayerNorms keep torch's defaults."""
        with torch.no_grad():
            for name, p in self.features.named_parameters():
                if p.dim() == 2:
                    nn.init.trunc_normal_(p, std=0.02)
                elif ".norm" not in name and not name.startswith("norm"):
                    p.zero_()
            nn.init.trunc_normal_(self.head.weight, std=0.02)
            self.head.bias.zero_()

    def blocks(self) -> List[SwinTransformerBlock]:
        """The transformer blocks in running order (the index k of p_k)."""
        return [b for i, stage in enumerate(self.features) if i % 2 == 0 for b in stage]

    def enable_training(self, stochastic_depth_prob: Optional[float] = None):
        """Make the encoder trainable (the reference's ``fix_bb: False``): requires_grad on every parameter ``forward`` uses
        (not ``norm.*`` / ``head.*``), ``forward`` with grad, and in ``.train()`` mode stochastic depth with
        p_k = stochastic_depth_prob * k / (n_blocks - 1) for block k.  None = the constructor's ``stochastic_depth_prob``
        (0.5 for ``swin_b()``, as in the reference); 0.0 switches stochastic depth off.  Call it before the optimiser's flat
        parameter buffer is built."""
        p = self.stochastic_depth_prob if stochastic_depth_prob is None else float(stochastic_depth_prob)
        if not 0.0 <= p < 1.0:
            raise ValueError(f"stochastic_depth_prob must be in [0, 1), got {p}")
        blocks = self.blocks()
        for k, b in enumerate(blocks):
            b.sd_prob = p * float(k) / max(len(blocks) - 1, 1)
        for name, q in self.named_parameters():
            q.requires_grad_(not (name.startswith("norm.") or name.startswith("head.")))
        self.trainable = True
        return self

    def draw_keep(self, batch: int, device) -> torch.Tensor:
        """[n_blocks, 2, batch] of 0. / 1.: the Bernoulli(1 - p_k) draws of one training forward (attention branch, MLP branch),
        from the device's generator."""
        p = torch.tensor([b.sd_prob for b in self.blocks()], device=device, dtype=torch.float32)
        return (torch.rand(p.numel(), 2, batch, device=device) >= p[:, None, None]).to(torch.float32)

    def forward(self, x, keep=None):
        """keep: the stochastic-depth draws ([n_blocks, 2, B] of 0 / 1; block k, branch, sample) in place of ``draw_keep()``:
        injectable for tests, used only by a trainable module in ``.train()`` mode and only where p_k > 0."""
        if not self.trainable:
            if keep is not None:
                raise RuntimeError("SwinTransformer: `keep` needs enable_training()")
            with torch.no_grad():
                return self._forward(x, None)
        return self._forward(x, keep)

    def _forward(self, x, keep):
        if self.training and not self.fix_bb and not self.trainable and not self._warned:
            self._warned = True
            warnings.warn("SwinTransformer: the backbone is frozen in this build (forward only, eval semantics) until "
                          "enable_training() is called (Unet(..., train_cond_encoder=True)); fix_bb: False alone does not train it")
        if x.dim() != 4 or x.shape[1] != self.in_chans:
            raise RuntimeError(f"the condition encoder takes an NCHW image with {self.in_chans} channels, got {tuple(x.shape)}")
        blocks = self.blocks()
        scales = None
        if self.trainable and self.training and any(b.sd_prob > 0.0 for b in blocks):
            hip.require_cuda(x, "x")
            if keep is None:
                keep = self.draw_keep(x.shape[0], x.device)
            if tuple(keep.shape) != (len(blocks), 2, x.shape[0]):
                raise RuntimeError(f"keep must be [{len(blocks)}, 2, {x.shape[0]}], got {tuple(keep.shape)}")
            inv = torch.tensor([1.0 / (1.0 - b.sd_prob) for b in blocks], device=x.device, dtype=torch.float32)
            scales = (keep.to(device=x.device, dtype=torch.float32) * inv[:, None, None]).contiguous()
        conv, ln = self.first_coonv[0], self.first_coonv[2]
        if self.in_chans == 1:
            h = osw.patch_embed_ln(x.to(torch.float32), conv.weight, conv.bias, ln.weight, ln.bias, ln.eps)
        else:
            h = oc.conv2d_generic(ops.nchw_to_nhwc(x.contiguous(), None, 32), conv.weight, conv.bias, stride=4, pad=0)
            h = osw.layer_norm(h, ln.weight, ln.bias, ln.eps)
        feats = []
        k = 0
        for i, layer in enumerate(self.features):
            if i % 2:
                h = layer(h)
                continue
            for b in layer:
                h = b(h, None if scales is None or b.sd_prob <= 0.0 else scales[k])
                k += 1
            feats.append(osw.nhwc_to_nchw(h))
        return feats


def load_encoder_weights(encoder: SwinTransformer, path: str) -> List[str]:
    """Start ``encoder`` from a LOCAL state dict (read with ``weights_only=True``; nothing is fetched): the ImageNet weights the
    reference's ``swin_b(weights=Swin_B_Weights...)`` starts from (swin_transformer.py:452-459).

    Two namings are read.  torchvision's own (``torchvision.models.swin_b().state_dict()``: the patch embedding is ``features.0``,
    the stages and mergings ``features.1`` ... ``features.7``) is recognised by its ``features.0.0.weight`` and renamed the way
    the reference pairs the two key lists in order (:455-457): ``features.0.{0,2}`` -> ``first_coonv.{0,2}``, ``features.k`` ->
    ``features.k-1``.  Otherwise the names are the encoder's own.  After that every ``features.*`` tensor of the encoder must be
    present with its shape, and no tensor of the file may be unknown or of another shape; ``first_coonv.*``, ``norm.*`` and
    ``head.*`` may be absent (they keep their initial values; a ``head`` of another class count is ignored).  Into a one-channel
    encoder a ``[E, 3, 4, 4]`` stem weight loads as its mean over the input channels (reference swin_transformer_for_sci.py
    :458-459); a ``[E, 1, 4, 4]`` one loads as it is.  Returns the names that were absent."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict) or not all(isinstance(v, torch.Tensor) for v in sd.values()):
        raise RuntimeError(f"{path}: expected a flat state dict of tensors")
    if "features.0.0.weight" in sd:          # torchvision's naming
        renamed = {}
        for k, v in sd.items():
            parts = k.split(".")
            if parts[0] == "features" and parts[1] == "0":
                k = ".".join(["first_coonv"] + parts[2:])
            elif parts[0] == "features":
                k = ".".join(["features", str(int(parts[1]) - 1)] + parts[2:])
            renamed[k] = v
        sd = renamed
    own = encoder.state_dict()
    stem = sd.get("first_coonv.0.weight")
    if stem is not None and encoder.in_chans == 1 and stem.dim() == 4 and stem.shape[1] == 3:
        sd = {**sd, "first_coonv.0.weight": stem.mean(dim=1, keepdim=True)}
    unknown = [k for k in sd if k not in own]
    if unknown:
        raise RuntimeError(f"{path}: {len(unknown)} tensors the encoder does not have (first: {unknown[0]})")
    if "head.weight" in sd and sd["head.weight"].shape != own["head.weight"].shape:
        sd = {k: v for k, v in sd.items() if not k.startswith("head.")}
    bad = [k for k, v in sd.items() if tuple(v.shape) != tuple(own[k].shape)]
    if bad:
        raise RuntimeError(f"{path}: {bad[0]} is {tuple(sd[bad[0]].shape)}, the encoder's is {tuple(own[bad[0]].shape)}")
    absent = [k for k in own if k not in sd]
    lost = [k for k in absent if k.startswith("features.")]
    if lost:
        raise RuntimeError(f"{path} lacks {len(lost)} of the encoder's features.* tensors (first: {lost[0]})")
    encoder.load_state_dict(sd, strict=False)
    return absent


def swin_b(**kwargs) -> SwinTransformer:
    """Swin-B: 4x4 patches, width 128, depths [2, 2, 18, 2], heads [4, 8, 16, 32], 7x7 windows.  No ``weights=`` argument: nothing
    is ever fetched, the tensors come from the conditional model's checkpoint."""
    return SwinTransformer(patch_size=[4, 4], embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], window_size=[7, 7],
                           **{"stochastic_depth_prob": 0.5, **kwargs})          # 0.5: reference :612-645, used after enable_training()
