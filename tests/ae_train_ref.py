"""Plain-PyTorch CPU restatement of the KL autoencoder's training step (TEST INFRASTRUCTURE ONLY), in whatever dtype its inputs
have (the tests use fp64, and fp32 to measure torch's own fp32 noise on the same inputs).

Restated from the reference: taming/modules/discriminator/model.py (NLayerDiscriminator, weights_init),
taming/modules/losses/vqperceptual.py (hinge_d_loss, adopt_weight), ddm/loss.py (LPIPSWithDiscriminator.forward,
calculate_adaptive_weight) and ddm/encoder_decoder.py:978-997 (AutoencoderKL.training_step).  The autoencoder itself is
oracle/ae_ref.py, the LPIPS network tests/lpips_ref.py (synthetic VGG16 weights around the real lin weights).

Everything is a pure function of flat state dicts with the reference's names: the autoencoder's (``encoder.*`` ...), and the
loss's (``logvar``, ``discriminator.main.N.*``; ``loss.`` in front of them inside an AutoencoderKL state dict).
"""
import torch
import torch.nn.functional as F

from oracle import ae_ref, fill

import lpips_ref


# ------------------------------------------------------------------------------------------------ PatchGAN discriminator
def disc_layers(input_nc=3, ndf=64, n_layers=3):
    """[(index in `main`, cin, cout, stride, has_bias, has_bn)] of NLayerDiscriminator(use_actnorm=False): every conv is 4x4, pad 1;
    BatchNorm2d sits at index + 1 and LeakyReLU(0.2) after every conv but the last."""
    out = [(0, input_nc, ndf, 2, True, False)]
    idx, mult = 2, 1
    for n in range(1, n_layers):
        prev, mult = mult, min(2 ** n, 8)
        out.append((idx, ndf * prev, ndf * mult, 2, False, True))
        idx += 3
    prev, mult = mult, min(2 ** n_layers, 8)
    out.append((idx, ndf * prev, ndf * mult, 1, False, True))
    out.append((idx + 3, ndf * mult, 1, 1, True, False))
    return out


def disc_shapes(input_nc=3, ndf=64, n_layers=3):
    """Names / shapes / order of NLayerDiscriminator.state_dict()."""
    s = {}
    for i, ci, co, _, bias, bn in disc_layers(input_nc, ndf, n_layers):
        s[f"main.{i}.weight"] = (co, ci, 4, 4)
        if bias:
            s[f"main.{i}.bias"] = (co,)
        if bn:
            s[f"main.{i + 1}.weight"] = (co,)
            s[f"main.{i + 1}.bias"] = (co,)
            s[f"main.{i + 1}.running_mean"] = (co,)
            s[f"main.{i + 1}.running_var"] = (co,)
            s[f"main.{i + 1}.num_batches_tracked"] = ()
    return s


def disc_state(wscale=1.0, input_nc=3, ndf=64, n_layers=3, tag="disc"):
    """Hash-filled discriminator state: conv weights uniform with the fan-in scale times `wscale` (the N(0, 0.02) of weights_init
    leaves the adaptive weight on its 1e4 clamp, which tests nothing), BN weights around 1, running statistics off their defaults."""
    sd = {}
    for k, shp in disc_shapes(input_nc, ndf, n_layers).items():
        leaf = k.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            sd[k] = torch.tensor(0, dtype=torch.long)
        elif leaf == "running_mean":
            sd[k] = fill.hash_tensor(shp, f"{tag}.{k}", 0.1)
        elif leaf == "running_var":
            sd[k] = 1.0 + fill.hash_tensor(shp, f"{tag}.{k}", 0.2)
        elif len(shp) == 1 and leaf == "weight":
            sd[k] = 1.0 + fill.hash_tensor(shp, f"{tag}.{k}", 0.2)
        elif leaf == "bias":
            sd[k] = fill.hash_tensor(shp, f"{tag}.{k}", 0.1)
        else:
            sd[k] = fill.hash_tensor(shp, f"{tag}.{k}", wscale * (3.0 / (shp[1] * 16)) ** 0.5)
    return sd


def discriminator(sd, x, training=True, p="", input_nc=3, ndf=64, n_layers=3, momentum=0.1, eps=1e-5):
    """NLayerDiscriminator.forward; in training mode the running statistics in `sd` are updated in place, as nn.BatchNorm2d does."""
    layers = disc_layers(input_nc, ndf, n_layers)
    h = x
    for i, _, _, stride, bias, bn in layers:
        h = F.conv2d(h, sd[f"{p}main.{i}.weight"], sd[f"{p}main.{i}.bias"] if bias else None, stride=stride, padding=1)
        if bn:
            q = f"{p}main.{i + 1}"
            h = F.batch_norm(h, sd[q + ".running_mean"], sd[q + ".running_var"], sd[q + ".weight"], sd[q + ".bias"], training,
                             momentum, eps)
            if training and q + ".num_batches_tracked" in sd:
                sd[q + ".num_batches_tracked"] += 1
        if i != layers[-1][0]:
            h = F.leaky_relu(h, 0.2)
    return h


def hinge_d_loss(logits_real, logits_fake):
    return 0.5 * (torch.mean(F.relu(1.0 - logits_real)) + torch.mean(F.relu(1.0 + logits_fake)))


def adopt_weight(weight, global_step, threshold=0, value=0.0):
    return value if global_step < threshold else weight


LOSS_DEFAULTS = dict(logvar_init=0.0, kl_weight=1.0, pixelloss_weight=1.0, disc_num_layers=3, disc_in_channels=3, disc_factor=1.0,
                     disc_weight=1.0, perceptual_weight=1.0)


def kl_per_sample(moments):
    mean, logvar = torch.chunk(moments, 2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    return 0.5 * torch.sum(mean ** 2 + torch.exp(logvar) - 1.0 - logvar, dim=[1, 2, 3])


def loss_forward(lsd, lp_sd, cfg, inputs, rec, moments, optimizer_idx, global_step, last_layer=None, training=True, split="train"):
    """LPIPSWithDiscriminator.forward (weights=None, cond=None, hinge).  lsd: the loss's state dict ('logvar',
    'discriminator.main.*'); lp_sd: LPIPS state dict or None (p_loss = 0).  Returns (loss, log)."""
    c = dict(LOSS_DEFAULTS, **cfg)
    B = inputs.shape[0]
    rec_loss = (inputs - rec).abs() + (inputs - rec) ** 2
    if c["perceptual_weight"] > 0 and lp_sd is not None:
        rec_loss = rec_loss + c["perceptual_weight"] * lpips_ref.lpips(lp_sd, inputs, rec).reshape(B, 1, 1, 1)
    logvar = lsd["logvar"]
    nll = rec_loss / torch.exp(logvar) + logvar
    nll_loss = torch.sum(nll) / B
    kl_loss = torch.sum(kl_per_sample(moments)) / B
    kw = dict(p="discriminator.", input_nc=c["disc_in_channels"], n_layers=c["disc_num_layers"])
    disc_factor = adopt_weight(c["disc_factor"], global_step, threshold=c["disc_start"])
    if optimizer_idx == 0:
        g_loss = -torch.mean(discriminator(lsd, rec, training, **kw))
        if c["disc_factor"] > 0.0:
            ng = torch.autograd.grad(nll_loss, last_layer, retain_graph=True)[0]
            gg = torch.autograd.grad(g_loss, last_layer, retain_graph=True)[0]
            d_weight = torch.clamp(torch.norm(ng) / (torch.norm(gg) + 1e-4), 0.0, 1e4).detach() * c["disc_weight"]
        else:
            d_weight = torch.tensor(0.0)
        loss = nll_loss + c["kl_weight"] * kl_loss + d_weight * disc_factor * g_loss
        log = {f"{split}/total_loss": loss.detach(), f"{split}/logvar": logvar.detach(), f"{split}/kl_loss": kl_loss.detach(),
               f"{split}/nll_loss": nll_loss.detach(), f"{split}/rec_loss": rec_loss.detach().mean(), f"{split}/d_weight": d_weight.detach(),
               f"{split}/disc_factor": torch.tensor(float(disc_factor)), f"{split}/g_loss": g_loss.detach()}
        return loss, log
    logits_real = discriminator(lsd, inputs.detach(), training, **kw)
    logits_fake = discriminator(lsd, rec.detach(), training, **kw)
    d_loss = disc_factor * hinge_d_loss(logits_real, logits_fake)
    log = {f"{split}/disc_loss": d_loss.detach(), f"{split}/logits_real": logits_real.detach().mean(),
           f"{split}/logits_fake": logits_fake.detach().mean()}
    return d_loss, log


def training_step(sd, cfg_ae, lp_sd, lossconfig, x, eps, optimizer_idx, global_step, training=True):
    """AutoencoderKL.training_step on the flat state dict `sd` (autoencoder names plus 'loss.logvar' / 'loss.discriminator.*')."""
    moments = ae_ref.encode_moments(sd, cfg_ae, x)
    rec = ae_ref.decode(sd, cfg_ae, ae_ref.posterior_sample(moments, eps))
    lsd = _LossView(sd)
    return loss_forward(lsd, lp_sd, lossconfig, x, rec, moments, optimizer_idx, global_step, last_layer=sd["decoder.conv_out.weight"],
                        training=training)


class _LossView:
    """The 'loss.'-prefixed entries of a state dict under their own names (reads and in-place writes go to the same tensors)."""

    def __init__(self, sd):
        self.sd = sd

    def __getitem__(self, k):
        return self.sd["loss." + k]

    def __setitem__(self, k, v):
        self.sd["loss." + k] = v

    def __contains__(self, k):
        return "loss." + k in self.sd


# ------------------------------------------------------------------------------------------------ fixed cases of the tests
CH, RES, BATCH = 32, (64, 64), 2
LOSSCONFIG = dict(disc_start=3, kl_weight=1e-6, disc_weight=0.5)


def ae_config():
    return ae_ref.ae_cfg(ch=CH, resolution=RES)


def full_state(wscale, dtype=torch.float64, logvar=0.0):
    """Autoencoder + loss state dict of a case, hash-filled; floating tensors in `dtype`."""
    sd = fill.filled_state_dict(ae_ref.param_shapes(ae_config()))
    sd["loss.logvar"] = torch.tensor(float(logvar))
    for k, v in disc_state(wscale).items():
        sd["loss.discriminator." + k] = v
    return {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def case_inputs(tag="main"):
    x = fill.hash_tensor((BATCH, 3, *RES), f"aet.{tag}.x", 1.0)
    eps = fill.hash_tensor((BATCH, 3, RES[0] // 4, RES[1] // 4), f"aet.{tag}.eps", 1.7)
    return x, eps


# scale of the discriminator's conv fill: with weights_init's N(0, 0.02) the adaptive weight sits on its 1e4 clamp (logged 5000 =
# 1e4 * 0.5), which tests nothing; WSCALE puts |grad nll| / |grad g| inside (1e-3, 1e3) (asserted by tools/make_golden_ae_train.py),
# WSCALE_CLAMP keeps one case on the clamp.  (Only the scale of the last conv and of the BatchNorm gains reaches the gradient at the
# discriminator's input: every other conv is followed by a BatchNorm in training mode, which cancels its scale.)  LOGVAR != 0 so
# that exp(-logvar) is not 1.
WSCALE, WSCALE_CLAMP, LOGVAR = 30.0, 1e-2, 2.0


def case_state(tag, dtype=torch.float64):
    """The state dict a case starts from: 'pre' / 'post' the plain fill; 'clamp' small discriminator weights; 'lvclamp' quant_conv
    biases that push the posterior's logvar beyond the [-30, 20] clamp on both sides."""
    sd = full_state(WSCALE_CLAMP if tag == "clamp" else WSCALE, dtype, LOGVAR)
    if tag == "lvclamp":
        sd["quant_conv.bias"] = sd["quant_conv.bias"].clone()
        sd["quant_conv.bias"][3:6] += torch.tensor([24.0, -34.0, 0.0], dtype=sd["quant_conv.bias"].dtype)
    return sd


GRAD_KEYS_SMALL = ("decoder.conv_out.weight", "encoder.conv_in.weight", "quant_conv.weight", "loss.logvar")
GRAD_KEYS = ("decoder.conv_out.weight", "encoder.conv_in.weight", "encoder.down.0.downsample.conv.weight",
             "encoder.mid.attn_1.q.weight", "encoder.mid.attn_1.k.weight", "encoder.mid.attn_1.v.weight",
             "encoder.mid.attn_1.proj_out.weight", "quant_conv.weight", "loss.logvar")
DISC_GRAD_KEYS = ("loss.discriminator.main.0.weight", "loss.discriminator.main.11.weight", "loss.discriminator.main.3.weight")


def step_with_grads(sd, lp_sd, lossconfig, x, eps, optimizer_idx, global_step, dtype=torch.float64):
    """Runs one training step in `dtype`; returns (loss, log, {name: gradient}) over the parameters that step trains, and leaves
    the updated BN running statistics in `sd`."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    stats = ("running_mean", "running_var", "num_batches_tracked")
    train = [k for k in sd if k.rsplit(".", 1)[-1] not in stats and
             (k.startswith("loss.discriminator.") == (optimizer_idx == 1)) and (optimizer_idx == 0 or k != "loss.logvar")]
    for k in train:
        sd[k] = sd[k].clone().requires_grad_(True)
    lp = None if lp_sd is None else lpips_ref.cast(lp_sd, dtype)
    loss, log = training_step(sd, ae_config(), lp, lossconfig, x.to(dtype), eps.to(dtype), optimizer_idx, global_step)
    grads = {}
    if loss.requires_grad:
        gs = torch.autograd.grad(loss, [sd[k] for k in train], allow_unused=True)
        grads = {k: g for k, g in zip(train, gs) if g is not None}
    return loss.detach(), log, grads, sd
