"""Plain-PyTorch CPU restatement of the LPIPS term (TEST INFRASTRUCTURE ONLY), in whatever dtype its inputs have (the tests use
fp64, and fp32 to measure the restatement's own noise).

Restated from the reference: taming/modules/losses/lpips.py:40-53 (forward), :56-63 (ScalingLayer), :75-112 (VGG16 slices),
:115-121 (normalize_tensor, spatial_average); ddm/ddm_const.py:326, 351-358 and ddm/ddm_const_2.py:217, 242-251 (x_rec and the
loss_vlb arithmetic).  It also makes SYNTHETIC VGG16 weights (hash-filled, He-scaled; the real ones cannot be fetched and are not
needed to check arithmetic) around the REAL five lin weights of tests/golden/lpips_lin.pt, and the fixed inputs of the GPU tests.
"""
import os

import torch
import torch.nn.functional as F

from oracle import fill

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
WIDTHS = ((3, 64, 64), (64, 128, 128), (128, 256, 256, 256), (256, 512, 512, 512), (512, 512, 512, 512))
CHNS = (64, 128, 256, 512, 512)


def lin_state_dict():
    return torch.load(os.path.join(GOLDEN, "lpips_lin.pt"), map_location="cpu", weights_only=True)


def vgg16_features_state_dict(tag="vgg"):
    """torchvision layout (features.N.weight / .bias): uniform hash fill with the He variance 2 / fan_in, biases around 0.05."""
    sd = {}
    for idx, w in zip(SLICES, WIDTHS):
        for j, i in enumerate(idx):
            ci, co = w[j], w[j + 1]
            sd[f"features.{i}.weight"] = fill.hash_tensor((co, ci, 3, 3), f"{tag}.features.{i}.weight", (6.0 / (ci * 9)) ** 0.5)
            sd[f"features.{i}.bias"] = 0.05 + fill.hash_tensor((co,), f"{tag}.features.{i}.bias", 0.03)
    return sd


def synthetic_state_dict(tag="vgg"):
    """The LPIPS module's own layout: scaling_layer.*, net.slice{k}.{i}.*, lin{k}.model.1.weight."""
    sd = {"scaling_layer.shift": torch.tensor([-.030, -.088, -.188])[None, :, None, None],
          "scaling_layer.scale": torch.tensor([.458, .448, .450])[None, :, None, None]}
    vgg = vgg16_features_state_dict(tag)
    for k, idx in enumerate(SLICES):
        for i in idx:
            for leaf in ("weight", "bias"):
                sd[f"net.slice{k + 1}.{i}.{leaf}"] = vgg[f"features.{i}.{leaf}"]
    sd.update(lin_state_dict())
    return sd


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def taps(sd, x):
    """VGG16 features of the scaled input: relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (NCHW)."""
    h = (x - sd["scaling_layer.shift"]) / sd["scaling_layer.scale"]
    out = []
    for k, idx in enumerate(SLICES):
        if k > 0:
            h = F.max_pool2d(h, 2, 2)
        for i in idx:
            h = F.relu(F.conv2d(h, sd[f"net.slice{k + 1}.{i}.weight"], sd[f"net.slice{k + 1}.{i}.bias"], padding=1))
        out.append(h)
    return out


def normalize_tensor(x, eps=1e-10):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


def head(f0, f1, w):
    """One tap: [B] = spatial mean of the 1x1 conv `w` [1,C,1,1] over (normalize(f0) - normalize(f1))^2."""
    d = (normalize_tensor(f0) - normalize_tensor(f1)) ** 2
    return F.conv2d(d, w).mean([2, 3]).reshape(-1)


def lpips(sd, x, target):
    """LPIPS.forward per sample, [B]."""
    f0, f1 = taps(sd, x), taps(sd, target)
    return sum(head(a, b, sd[f"lin{k}.model.1.weight"]) for k, (a, b) in enumerate(zip(f0, f1)))


def x_rec(schedule, C_pred, noise_pred, x_noisy, t):
    if schedule == "const":
        return -1 * C_pred
    tt = t.reshape(-1, 1, 1, 1)
    return x_noisy - C_pred * tt - tt * noise_pred


def loss_vlb(per_sample, t):
    """[B] * [B,1] -> [B,B], summed and divided by B: the product of the two sums / B."""
    rec_weight = -torch.log(t.reshape(-1, 1)) / 2
    return (per_sample * rec_weight).sum() / t.shape[0]


# ---------------------------------------------------------------------------------------------------------------------------
# fixed inputs of the GPU tests; tests/test_lpips_host.py checks their conditioning (fp32 against fp64) on the CPU
# ---------------------------------------------------------------------------------------------------------------------------
# (B, size, seed).  Seed 0 at 32x32 fails the host test's condition (fp32 against fp64 d/dx: 2.3e-4 relative L2, one ReLU / pool
# flip; seeds 1..5 measure 2.2e-6 at 32x32, and 2.6e-6 at 64x64 but for seed 5's 4.4e-5), so seed 1 it is.
NETWORK_CASES = ((4, 32, 1), (4, 64, 1))


def network_inputs(B, size, seed):
    """x0 in [-1, 1] and x_rec = x0 + 0.3 N(0, 1), fp32 NCHW."""
    x0 = fill.hash_tensor((B, 3, size, size), f"lpips.x0.{size}.{seed}", 1.0)
    g = torch.Generator().manual_seed(1000 + seed)
    return x0 + 0.3 * torch.randn(x0.shape, generator=g), x0


def value_and_grad(sd, x, target, dtype):
    """(per-sample values, d sum_b lpips_b / d x, taps of x) in `dtype`."""
    sdd = cast(sd, dtype)
    xr = x.to(dtype).clone().requires_grad_(True)
    per = lpips(sdd, xr, target.to(dtype))
    (g,) = torch.autograd.grad(per.sum(), xr)
    with torch.no_grad():
        tp = taps(sdd, xr)
    return per.detach(), g, tp


def conditioning(sd, x, target):
    """fp32 restatement against fp64 on one input set: (largest relative gap of the per-sample values, relative L2 gap of d/dx,
    number of tap positions of x whose feature vector is all zero)."""
    p64, g64, t64 = value_and_grad(sd, x, target, torch.float64)
    p32, g32, _ = value_and_grad(sd, x, target, torch.float32)
    rel = float(((p32.double() - p64).abs() / p64.abs()).max())
    grel = float((g32.double() - g64).norm() / g64.norm())
    zeros = sum(int((f.abs().amax(dim=1) == 0).sum()) for f in t64)
    return rel, grel, zeros


# ---------------------------------------------------------------------------------------------------------------------------
# wrapper level: the small UNet of smoke() (model_channels=64, num_blocks=1, oracle.fill weights), fixed t and noise
# ---------------------------------------------------------------------------------------------------------------------------
WRAPPER = {"const": ("uncond_unet", 1e-4), "const_2": ("uncond_unet_sd_2", 1e-3)}        # schedule -> (UNet variant, eps)
GRAD_KEY = "model.enc.16x16_block0.conv1.weight"


def wrapper_inputs():
    x0 = fill.hash_tensor((2, 3, 32, 32), "x0", 1.0)
    noise = fill.hash_tensor((2, 3, 32, 32), "noise", 1.7)
    return x0, noise, torch.tensor([0.23, 0.81])


def small_unet(schedule):
    from oracle import unet_ref
    cfg = unet_ref.default_cfg(variant=WRAPPER[schedule][0], model_channels=64, num_blocks=1, dropout=0.0)
    return cfg, fill.filled_state_dict(unet_ref.param_shapes(cfg))


def oracle_step(schedule, lp_sd, lp_dtype=torch.float64):
    """oracle.ddm_ref.p_losses (fp32 UNet oracle) plus the restatement, in `lp_dtype`, applied to the oracle's own predictions.
    Returns the three logged values' sources, the parameter gradients of the full loss and the gradient of the LPIPS term alone
    with respect to GRAD_KEY."""
    from oracle import ddm_ref, unet_ref
    cfg, sd = small_unet(schedule)
    x0, noise, t = wrapper_inputs()
    sdo = {k: v.clone().requires_grad_("resample" not in k) for k, v in sd.items()}
    mf = lambda x, tt, **k: unet_ref.edm_precond(sdo, cfg, x, tt, **k)
    loss_simple, log, (x_noisy, C_pred, noise_pred) = ddm_ref.p_losses(schedule, mf, x0, t, noise, WRAPPER[schedule][1], True)
    xr = x_rec(schedule, C_pred.to(lp_dtype), noise_pred.to(lp_dtype), x_noisy.to(lp_dtype), t.to(lp_dtype))
    per = lpips(cast(lp_sd, lp_dtype), xr, x0.to(lp_dtype))
    vlb = loss_vlb(per, t.to(lp_dtype))
    (g_vlb,) = torch.autograd.grad(vlb, sdo[GRAD_KEY], retain_graph=True)
    loss = loss_simple.to(lp_dtype) + vlb
    loss.backward()
    n = x0[0].numel()
    return {"loss": loss.detach(), "log_loss_simple": log["train/loss_simple"], "log_loss_vlb": vlb.detach() / n,
            "vlb": vlb.detach(), "per": per.detach(), "x_rec": xr.detach().to(torch.float32),
            "grads": {k: v.grad for k, v in sdo.items() if v.grad is not None}, "g_vlb": g_vlb}
