"""The ONE-channel cases of the KL autoencoder's training step (TEST INFRASTRUCTURE ONLY): AutoencoderKL(in_channels=1, out_ch=1)
with LPIPSWithDiscriminator(disc_in_channels=1), the first stage of the latent saliency recipe.  Everything that computes is
tests/ae_train_ref.py's (whose functions take the channel counts as arguments); this file holds the cases' shapes, fills and the
one-channel ``step_with_grads``.

ch = 32, B = 2, 64x48: NON-SQUARE on purpose, so that an H / W mix-up in a one-channel layout kernel shows; the mid attention has
L = 16 x 12 = 192 tokens, and H, W are multiples of 16 (the training path's rule).  The LPIPS network sees the one channel
broadcast to three by its ScalingLayer (tests/lpips_ref.py taps: (x - shift[1,3,1,1]) / scale).
"""
import torch

from oracle import ae_ref, fill

import ae_train_ref as R
import lpips_ref

CH, RES, BATCH = 32, (64, 48), 2
LOSSCONFIG = dict(R.LOSSCONFIG, disc_in_channels=1)
WSCALE, LOGVAR = R.WSCALE, R.LOGVAR
STEPS = {"pre": 0, "post": 3}
CASES = [("pre", 0), ("pre", 1), ("post", 0), ("post", 1)]


def grad_keys(tag, idx):
    """The gradients g27 records: the full lists at 'post', the short ones at 'pre' (as g18 does)."""
    if idx == 0:
        return R.GRAD_KEYS if tag == "post" else R.GRAD_KEYS_SMALL
    return R.DISC_GRAD_KEYS if tag == "post" else R.DISC_GRAD_KEYS[:1]


def ae_config():
    return ae_ref.ae_cfg(ch=CH, resolution=RES, in_channels=1, out_ch=1)


def full_state(wscale=WSCALE, dtype=torch.float64, logvar=LOGVAR):
    """Autoencoder + loss state dict, hash-filled (tags of their own: not the three-channel cases' numbers)."""
    sd = fill.filled_state_dict(ae_ref.param_shapes(ae_config()))
    sd["loss.logvar"] = torch.tensor(float(logvar))
    for k, v in R.disc_state(wscale, input_nc=1, tag="disc.c1").items():
        sd["loss.discriminator." + k] = v
    return {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def case_state(tag, dtype=torch.float64):
    return full_state(WSCALE, dtype, LOGVAR)


def case_inputs(tag):
    x = fill.hash_tensor((BATCH, 1, *RES), f"aet.c1.{tag}.x", 1.0)
    eps = fill.hash_tensor((BATCH, 3, RES[0] // 4, RES[1] // 4), f"aet.c1.{tag}.eps", 1.7)
    return x, eps


def step_with_grads(sd, lp_sd, lossconfig, x, eps, optimizer_idx, global_step, dtype=torch.float64):
    """ae_train_ref.step_with_grads on the one-channel configuration."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    stats = ("running_mean", "running_var", "num_batches_tracked")
    train = [k for k in sd if k.rsplit(".", 1)[-1] not in stats and
             (k.startswith("loss.discriminator.") == (optimizer_idx == 1)) and (optimizer_idx == 0 or k != "loss.logvar")]
    for k in train:
        sd[k] = sd[k].clone().requires_grad_(True)
    lp = None if lp_sd is None else lpips_ref.cast(lp_sd, dtype)
    loss, log = R.training_step(sd, ae_config(), lp, lossconfig, x.to(dtype), eps.to(dtype), optimizer_idx, global_step)
    grads = {}
    if loss.requires_grad:
        gs = torch.autograd.grad(loss, [sd[k] for k in train], allow_unused=True)
        grads = {k: g for k, g in zip(train, gs) if g is not None}
    return loss.detach(), log, grads, sd
