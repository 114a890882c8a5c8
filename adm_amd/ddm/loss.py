"""Training loss of the KL autoencoder on the HIP hot path: LPIPS + PatchGAN discriminator with the adaptive weight.

Restated from the reference's ddm/loss.py (LPIPSWithDiscriminator), taming/modules/discriminator/model.py (NLayerDiscriminator,
weights_init) and taming/modules/losses/vqperceptual.py (hinge_d_loss, adopt_weight).  State-dict layout as there, so state dicts
interchange: ``logvar``, ``discriminator.main.{0,2,3,5,6,8,9,11}.*`` and, once installed, ``perceptual_loss.*``.

The ``nn.Conv2d`` / ``nn.BatchNorm2d`` objects are parameter containers; the arithmetic runs through adm_amd.ops_cond
(BatchNorm) and adm_amd.ops_ae (the 4x4 convs: the kernels of ops_cond.conv2d_generic with cached packed weights and a weight
gradient that ADM_DETERMINISTIC=1 makes bit-reproducible; LeakyReLU, the hinge / generator terms, the NLL term, the adaptive weight) on NHWC fp32
buffers.  f32 compute mode only.

The reference takes ``torch.autograd.grad`` of the NLL and of the generator loss with respect to the decoder's last layer.  Here
the generator step is explicit (``generator_step``): both gradients are taken at the (detached) reconstruction, the last layer's
weight-gradient kernel runs on each, the two norms give the device scalar ``d_weight``, and ONE backward pass carries
``g_nll + d_weight * disc_factor * g_gan`` through decoder, posterior and encoder.  Nothing is copied to the host.
"""
from __future__ import annotations

import contextlib
import warnings
from typing import Optional

import torch
import torch.nn as nn

from .. import hip, ops, ops_ae, ops_cond
from .lpips import LPIPS


def adopt_weight(weight, global_step, threshold=0, value=0.0):
    return value if global_step < threshold else weight


def weights_init(m):
    name = m.__class__.__name__
    if name.find("Conv") != -1:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif name.find("BatchNorm") != -1:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


class NLayerDiscriminator(nn.Module):
    """PatchGAN discriminator: 4x4 convs (stride 2, the last two stride 1), BatchNorm2d, LeakyReLU(0.2).  Input and output are
    NHWC with channels padded to 32: [B,H,W,32] -> the logit map [B,h,w,32] whose channel 0 is the logit."""

    def __init__(self, input_nc=3, ndf=64, n_layers=3, use_actnorm=False):
        super().__init__()
        if use_actnorm:
            raise NotImplementedError("use_actnorm=True (ActNorm in the discriminator) is not implemented; no DDM recipe uses it")
        seq = [nn.Conv2d(input_nc, ndf, kernel_size=4, stride=2, padding=1), nn.LeakyReLU(0.2, True)]
        mult = 1
        for n in range(1, n_layers):
            prev, mult = mult, min(2 ** n, 8)
            seq += [nn.Conv2d(ndf * prev, ndf * mult, kernel_size=4, stride=2, padding=1, bias=False), nn.BatchNorm2d(ndf * mult),
                    nn.LeakyReLU(0.2, True)]
        prev, mult = mult, min(2 ** n_layers, 8)
        seq += [nn.Conv2d(ndf * prev, ndf * mult, kernel_size=4, stride=1, padding=1, bias=False), nn.BatchNorm2d(ndf * mult),
                nn.LeakyReLU(0.2, True)]
        seq += [nn.Conv2d(ndf * mult, 1, kernel_size=4, stride=1, padding=1)]
        self.main = nn.Sequential(*seq)         # containers only: `main` is never called

    def forward(self, x):
        h = x
        for m in self.main:
            if isinstance(m, nn.Conv2d):
                h = ops_ae.conv2d_down(h, m.weight, m.bias, stride=m.stride[0], pad_lo=m.padding[0], pad_hi=m.padding[0])
            elif isinstance(m, nn.BatchNorm2d):
                h = ops_cond.batch_norm(h, m, self.training)
            else:
                h = ops_ae.leaky_relu(h, m.negative_slope)
        return h


@contextlib.contextmanager
def _frozen(module: nn.Module):
    """Parameters of `module` take no gradient inside: the data gradient passes, no weight-gradient kernel is launched."""
    ps = [p for p in module.parameters() if p.requires_grad]
    for p in ps:
        p.requires_grad_(False)
    try:
        yield
    finally:
        for p in ps:
            p.requires_grad_(True)


def last_layer_gradient(h_last, g_nchw, conv: nn.Conv2d):
    """d / d conv.weight of a loss whose gradient at the NCHW output of `conv` (3x3, pad 1) is g_nchw, from the conv's saved NHWC
    input h_last: the weight-gradient kernel alone, into a fresh OIHW buffer (neither .grad nor the flat buffer is touched)."""
    B, H, W, cip = h_last.shape
    co, ci, ks = conv.weight.shape[0], conv.weight.shape[1], conv.weight.shape[-1]
    cop = ops.ceil32(co)
    dy = ops._nchw_to_nhwc(g_nchw.contiguous(), None, cop)
    dw = torch.empty_like(conv.weight)
    if ops.DETERMINISTIC:          # pixel-range partials to a workspace, summed in split order
        splits = hip.lib().adm_conv_wgrad_plan(B, H, W, cip, cop, ks, 0, 0)
        if splits < 1:
            raise RuntimeError(f"adm_conv_wgrad_plan failed with code {splits}")
        ws = torch.empty((splits, cop, ks * ks * cip), device=dy.device, dtype=torch.float32)
        hip.call("adm_conv_wgrad_ws", hip.ptr(h_last), hip.ptr(dy), hip.ptr(ws), None, B, H, W, cip, cip, cop, cop, ks, 0, splits, 0)
        hip.call("adm_unpack_wgrad_splits", hip.ptr(ws), splits, hip.ptr(dw), co, ci, ks, cop, cip, 0, 0, None, None)
    else:
        dwp = torch.empty((cop, ks * ks * cip), device=dy.device, dtype=torch.float32)
        hip.call("adm_conv_wgrad", hip.ptr(h_last), hip.ptr(dy), hip.ptr(dwp), B, H, W, cip, cip, cop, cop, ks, 0, 0)
        hip.call("adm_unpack_wgrad", hip.ptr(dwp), hip.ptr(dw), co, ci, ks, cop, cip, 0, 0)
    return dw


class TrainingPosterior:
    """What AutoencoderKL's training forward hands to the loss where the reference passes its posterior object: the per-sample KL
    (with its graph), the detached input ``h_last`` of the decoder's last conv ``conv_out``.  ``forward(optimizer_idx=0)`` leaves
    the gradients it produced here: ``g`` = d loss / d reconstruction (NCHW) and ``dlogvar`` = d loss / d logvar."""

    def __init__(self, kl, h_last, conv_out):
        self.kl_per_sample, self.h_last, self.conv_out = kl, h_last, conv_out
        self.g = self.dlogvar = None

    def kl(self):
        return self.kl_per_sample


class LPIPSWithDiscriminator(nn.Module):
    def __init__(self, *, disc_start, logvar_init=0.0, kl_weight=1.0, pixelloss_weight=1.0, disc_num_layers=3, disc_in_channels=3,
                 disc_factor=1.0, disc_weight=1.0, perceptual_weight=1.0, use_actnorm=False, disc_conditional=False,
                 disc_loss="hinge", lpips_ckpt=None):
        super().__init__()
        if disc_loss not in ("hinge", "vanilla"):
            raise ValueError(f"disc_loss {disc_loss!r}")
        if disc_loss == "vanilla":
            raise NotImplementedError('disc_loss="vanilla" is not implemented (every DDM recipe uses the hinge loss)')
        if disc_conditional:
            raise NotImplementedError("disc_conditional=True is not implemented (no DDM recipe conditions the discriminator)")
        self.kl_weight = kl_weight
        self.pixel_weight = pixelloss_weight
        self.perceptual_weight = perceptual_weight
        self.perceptual_loss: Optional[LPIPS] = None          # no weights ship and none are fetched: see set_perceptual_loss
        self.logvar = nn.Parameter(torch.ones(size=()) * logvar_init)
        self.discriminator = NLayerDiscriminator(input_nc=disc_in_channels, n_layers=disc_num_layers,
                                                 use_actnorm=use_actnorm).apply(weights_init)
        self.discriminator_iter_start = disc_start
        self.disc_factor = disc_factor
        self.discriminator_weight = disc_weight
        self.disc_conditional = disc_conditional
        self._warned = False
        if lpips_ckpt is not None:
            self.set_perceptual_loss(LPIPS.from_file(lpips_ckpt))

    def set_perceptual_loss(self, lpips: Optional[LPIPS]):
        """Installs (or, with None, removes) the frozen LPIPS network; its weights then appear as ``perceptual_loss.*``."""
        self.perceptual_loss = None if lpips is None else lpips.to(self.logvar.device).eval()
        return self

    def _p_loss(self, inputs, rec):
        if not self.perceptual_weight > 0:
            return None
        if self.perceptual_loss is None:
            if not self._warned:
                warnings.warn("LPIPSWithDiscriminator: perceptual_weight > 0 but no LPIPS weights are installed (a checkpoint's "
                              "loss.perceptual_loss.* keys, lossconfig lpips_ckpt, or set_perceptual_loss()); using p_loss = 0")
                self._warned = True
            return None
        # LPIPS.forward differentiates its FIRST argument only; the distance is symmetric, so the reconstruction goes first
        return self.perceptual_loss(rec, inputs)

    def _check(self, weights, cond):
        if weights is not None:
            raise NotImplementedError("weights= (per-element NLL weights) is not implemented")
        if cond is not None:
            raise NotImplementedError("a conditional discriminator (cond=) is not implemented")
        if ops.COMPUTE != "f32":
            raise NotImplementedError("the autoencoder trains in the f32 compute mode only (bf16 mode is not implemented)")

    # ------------------------------------------------------------------------------------------- generator side
    def generator_step(self, inputs, rec, h_last, conv_out, kl, global_step, split="train"):
        """optimizer_idx == 0 at the detached reconstruction.  inputs, rec: NCHW (rec without a graph); h_last: the saved NHWC input
        of the decoder's last conv `conv_out`; kl [B].  Returns (loss, log, g, dlogvar): g = d loss / d rec (NCHW) with the adaptive
        weight applied and dlogvar = d loss / d logvar, both device tensors; the KL term's gradient is the caller's
        (kl_weight / B per sample)."""
        B = inputs.shape[0]
        rec = rec.detach().requires_grad_(True)
        with torch.enable_grad():
            out = ops_ae.nll_terms(inputs, rec, self._p_loss(inputs, rec), self.logvar, self.perceptual_weight)
            (g_nll,) = torch.autograd.grad(out[0], rec)
            with _frozen(self.discriminator):
                logits_fake = self.discriminator(ops.nchw_to_nhwc(rec, None, ops.ceil32(rec.shape[1])))
                g_loss = -ops_ae.logit_mean(logits_fake)
                (g_gan,) = torch.autograd.grad(g_loss, rec)
        out, g_loss = out.detach(), g_loss.detach()
        if self.disc_factor > 0.0:
            d_weight = ops_ae.adaptive_weight(last_layer_gradient(h_last, g_nll, conv_out), last_layer_gradient(h_last, g_gan, conv_out),
                                              self.discriminator_weight)
        else:
            d_weight = torch.zeros((), device=rec.device)
        disc_factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
        g = ops_ae.axpy_dev(g_nll, g_gan, d_weight, disc_factor)
        kl_loss = kl.detach().sum() / B
        nll_loss = out[0]
        loss = nll_loss + self.kl_weight * kl_loss + d_weight * disc_factor * g_loss
        log = {f"{split}/total_loss": loss, f"{split}/logvar": self.logvar.detach(), f"{split}/kl_loss": kl_loss,
               f"{split}/nll_loss": nll_loss, f"{split}/rec_loss": out[1], f"{split}/d_weight": d_weight,
               f"{split}/disc_factor": torch.tensor(float(disc_factor)), f"{split}/g_loss": g_loss}
        return loss, log, g, out[2]

    # ------------------------------------------------------------------------------------------- discriminator side
    def discriminator_loss(self, inputs, rec, global_step, split="train"):
        """optimizer_idx == 1: two separate discriminator calls, real then fake, each with its own batch statistics and its own
        running-statistics update.  The returned loss carries the graph of the discriminator."""
        c = ops.ceil32(inputs.shape[1])
        logits_real = self.discriminator(ops.nchw_to_nhwc(inputs.detach(), None, c))
        logits_fake = self.discriminator(ops.nchw_to_nhwc(rec.detach(), None, c))
        disc_factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
        d_loss = disc_factor * 0.5 * (ops_ae.hinge_real(logits_real) + ops_ae.hinge_fake(logits_fake))
        log = {f"{split}/disc_loss": d_loss.detach(), f"{split}/logits_real": ops_ae.logit_mean(logits_real.detach()),
               f"{split}/logits_fake": ops_ae.logit_mean(logits_fake.detach())}
        return d_loss, log

    def forward(self, inputs, reconstructions, posteriors, optimizer_idx, global_step, last_layer=None, cond=None, split="train",
                weights=None):
        """The reference's signature; returns (loss, log).  optimizer_idx == 1: the discriminator loss with its graph
        (`posteriors` is not used).  optimizer_idx == 0 cannot be a graph loss here (``autograd.grad`` with respect to the last
        layer is not available: a parameter of the flat gradient buffer receives its gradient outside autograd), so the loss is
        returned as a VALUE and the gradients of the explicit generator step are left in `posteriors`, a TrainingPosterior, for
        AutoencoderKL.training_step to send through decoder, posterior and encoder.  `last_layer` is accepted for the signature;
        the layer is `posteriors.conv_out`."""
        self._check(weights, cond)
        if optimizer_idx == 1:
            return self.discriminator_loss(inputs, reconstructions, global_step, split)
        if optimizer_idx != 0:
            raise ValueError(f"optimizer_idx {optimizer_idx}")
        if not isinstance(posteriors, TrainingPosterior):
            raise TypeError("optimizer_idx == 0 needs the TrainingPosterior of AutoencoderKL's training forward (use "
                            "AutoencoderKL.training_step)")
        loss, log, posteriors.g, posteriors.dlogvar = self.generator_step(inputs, reconstructions, posteriors.h_last,
                                                                          posteriors.conv_out, posteriors.kl(), global_step, split)
        return loss, log
