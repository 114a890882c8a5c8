"""LPIPS (VGG16) perceptual distance as a frozen module on the HIP hot path.

Restated from the reference's taming/modules/losses/lpips.py: ScalingLayer (:56-63), the five slices of torchvision's VGG16
``features`` (:75-112), ``normalize_tensor`` / ``spatial_average`` (:115-121) and the five 1x1 ``lin`` layers (:66-72) summed in
``LPIPS.forward`` (:40-53).  The state-dict layout is the reference's, so state dicts interchange:

  scaling_layer.shift / .scale              buffers [1,3,1,1]
  net.slice1.{0,2}  net.slice2.{5,7}  net.slice3.{10,12,14}  net.slice4.{17,19,21}  net.slice5.{24,26,28}   .weight / .bias
  lin{0..4}.model.1.weight                  [1, C_k, 1, 1]   (index 1: a Dropout sits at index 0 in the reference; it is inactive
                                                              in .eval(), which is how the loss uses the network, so none here)

No weights ship with this package and nothing is ever fetched: they come from a reference-trained checkpoint (its state dict
carries ``perceptual_loss.*``) or from local files (a torchvision VGG16 state dict plus the reference's 7 KB ``vgg.pth``).

The thirteen 3x3 convs run through ``ops.conv2d`` in NHWC with channels padded to 32; the weights are frozen, so the backward is
the data gradient alone.  The fused input kernel, the 2x2 max-pool and the normalise / difference / lin / mean head are
csrc/lpips.hip.  Every tapped feature map feeds its head and the next slice: ``ops.fanout`` splits it, so the gradient sum is the
project's kernel.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn as nn

from .. import ops, ops_cond

# (index in torchvision's vgg16().features, cin, cout) per slice; a MaxPool2d(2, 2) opens slices 2..5 (features 4, 9, 16, 23)
SLICES = (((0, 3, 64), (2, 64, 64)),
          ((5, 64, 128), (7, 128, 128)),
          ((10, 128, 256), (12, 256, 256), (14, 256, 256)),
          ((17, 256, 512), (19, 512, 512), (21, 512, 512)),
          ((24, 512, 512), (26, 512, 512), (28, 512, 512)))
CHNS = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
PREFIX = "perceptual_loss."


class _Frozen(nn.Module):
    """weight (and bias) holder with the reference's parameter names; never trained."""

    def __init__(self, wshape, bias: bool):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(wshape), requires_grad=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(wshape[0]), requires_grad=False)


def _holder(children: Dict[str, nn.Module]) -> nn.Module:
    m = nn.Module()
    for k, v in children.items():
        m.add_module(k, v)
    return m


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(SCALE)[None, :, None, None])


class LPIPS(nn.Module):
    def __init__(self):
        super().__init__()
        self.scaling_layer = ScalingLayer()
        self.net = _holder({f"slice{k + 1}": _holder({str(i): _Frozen((co, ci, 3, 3), True) for i, ci, co in sl})
                            for k, sl in enumerate(SLICES)})
        for k, c in enumerate(CHNS):
            self.add_module(f"lin{k}", _holder({"model": _holder({"1": _Frozen((1, c, 1, 1), False)})}))
        self.eval()

    def train(self, mode: bool = True):
        return super().train(False)        # frozen, as the reference's disabled_train

    # ------------------------------------------------------------------ loaders
    @classmethod
    def from_state_dict(cls, sd: Dict[str, torch.Tensor]) -> "LPIPS":
        """From a state dict in the layout above, with or without the ``perceptual_loss.`` prefix (a reference-trained checkpoint's
        own keys); other keys of a prefixed dict are ignored."""
        if any(k.startswith(PREFIX) for k in sd):
            sd = {k[len(PREFIX):]: v for k, v in sd.items() if k.startswith(PREFIX)}
        m = cls()
        m.load_state_dict(sd, strict=True)
        return m

    @classmethod
    def from_vgg16(cls, vgg_sd: Dict[str, torch.Tensor], lin_sd: Dict[str, torch.Tensor]) -> "LPIPS":
        """From a torchvision-layout VGG16 state dict (``features.N.weight/bias``; classifier keys are ignored) and the ``lin*``
        state dict of the reference's taming/modules/autoencoder/lpips/vgg.pth."""
        sd = {}
        for k, sl in enumerate(SLICES):
            for i, _, _ in sl:
                for leaf in ("weight", "bias"):
                    sd[f"net.slice{k + 1}.{i}.{leaf}"] = vgg_sd[f"features.{i}.{leaf}"]
        for k in range(len(CHNS)):
            sd[f"lin{k}.model.1.weight"] = lin_sd[f"lin{k}.model.1.weight"]
        m = cls()
        m.load_state_dict(sd, strict=False)      # (the scaling-layer buffers are constants)
        return m

    @classmethod
    def from_file(cls, path: str, lin_path: Optional[str] = None) -> "LPIPS":
        """``path``: a state dict in this module's layout (plain, prefixed, or under a checkpoint's 'model' key), or -- with
        ``lin_path`` -- a torchvision VGG16 state dict next to the reference's lin file."""
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if "model" in sd and isinstance(sd["model"], dict):
            sd = sd["model"]
        if lin_path is not None:
            return cls.from_vgg16(sd, torch.load(lin_path, map_location="cpu", weights_only=True))
        return cls.from_state_dict(sd)

    # ------------------------------------------------------------------ forward
    def features(self, h: torch.Tensor, split: bool):
        """The five taps (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3) of the scaled NHWC input h [B,H,W,32]."""
        if ops.COMPUTE != "f32":
            raise NotImplementedError("the LPIPS branch runs in the f32 compute mode only")
        B, H, W, _ = h.shape
        if H % 16 or W % 16:
            raise NotImplementedError(f"LPIPS needs H and W that are multiples of 16 (four 2x2 pools), got {H}x{W}")
        taps = []
        for k, sl in enumerate(SLICES):
            if k > 0:
                h = ops.maxpool2x2(h)
            mods = getattr(self.net, f"slice{k + 1}")
            for i, _, _ in sl:
                conv = getattr(mods, str(i))
                h = ops_cond.relu_dropout(ops.conv2d(h, conv.weight, conv.bias), 0.0)
            if split and k + 1 < len(SLICES):
                tap, h = ops.fanout(h, 2)        # two consumers: the head and the next slice
            else:
                tap = h
            taps.append(tap)
        return taps

    def _heads(self, inp, tgt):
        with torch.no_grad():
            f1 = self.features(tgt, False)
        f0 = self.features(inp, True)
        return ops.lpips_heads(f0, f1, [getattr(getattr(self, f"lin{k}").model, "1").weight for k in range(len(CHNS))])

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """LPIPS(input, target) per sample, [B]; NCHW images as in the reference (whose result is [B,1,1,1]).  Differentiable in
        ``input`` only: the loss never differentiates its target."""
        sl = self.scaling_layer
        tgt = ops.lpips_input(target.detach(), None, None, None, sl.shift, sl.scale, -1)
        return self._heads(ops.lpips_input(input, None, None, None, sl.shift, sl.scale, -1), tgt)

    def from_predictions(self, C_pred, noise_pred, x_noisy, t, x_start, schedule: int) -> torch.Tensor:
        """LPIPS(x_rec, x_start) [B] with x_rec rebuilt from the denoiser's predictions inside the input kernel: schedule 0
        ('const') x_rec = -C_pred; 1 ('const_2') x_rec = x_noisy - C_pred t - t noise_pred."""
        sl = self.scaling_layer
        tgt = ops.lpips_input(x_start.detach(), None, None, None, sl.shift, sl.scale, -1)
        return self._heads(ops.lpips_input(C_pred, noise_pred, x_noisy, t, sl.shift, sl.scale, schedule), tgt)
