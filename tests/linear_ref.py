"""Plain-PyTorch CPU restatement of the linear-drift DDM wrapper (TEST INFRASTRUCTURE ONLY), in whatever dtype its inputs have
(the GPU tests use fp64; the fixture generator runs it in fp32 against the imported reference).

Written from the behaviour of the reference's ddm/ddm_linear.py ``DDPM``:

  * U(t) = K t^2/2 + C t with C = -x0 - K/2, K clamped to [-1, 1];  x_t = x0 + U(t) + sqrt(t) eps;
  * the denoiser returns theta_pred = [K_pred | C_pred] (six channels) and noise_pred; x_rec = x_t - K_pred t^2/2 - C_pred t - sqrt(t) noise_pred;
  * loss_simple = mean_b [w1 mean (theta_pred - [K|C])^2 + w2 mean (noise_pred - eps)^2], with use_l1 the mean-|.| twins added and the
    sum halved; w1 = 1/t, w2 = 1/(1 - t + eps) under weighting_loss;
  * loss_vlb = mean over the [B,B] product of (MAE_b [+ LPIPS_b]) [B] and (1 - t_b)^2 [B,1];
  * the sampler: fp32 step sizes n x 1/n (with denoise the last one split into 1/n - eps and eps), the last step takes s = cur_time;
    K_pred is clamped; x <- x + K s^2/2 - K t s - C s - s/sqrt(t) noise_pred + sqrt(s (t - s)/t) z; then clamp to +-scale_input,
    / scale_input, (x + 1)/2;
  * the UNet with ``precondition=False`` still sees c_in * x and log t; only the output combination is dropped.
"""
import torch

from oracle import fill, unet_ref

FULL = dict(variant="uncond_unet", dropout=0.0)                                    # 192 wide, [1,2,2,2], 3 blocks
SMALL = dict(variant="uncond_unet", model_channels=64, num_blocks=1, dropout=0.0)


def cfg_and_shapes(**over):
    """The UNet config and the parameter shapes of its out_mul = 2 form (model.out_conv.* has six outputs)."""
    cfg = unet_ref.default_cfg(**over)
    shapes = dict(unet_ref.param_shapes(cfg))
    w = shapes["model.out_conv.weight"]
    shapes["model.out_conv.weight"] = (2 * w[0],) + tuple(w[1:])
    shapes["model.out_conv.bias"] = (2 * w[0],)
    return cfg, shapes


def unet(sd, cfg, x, t, augment_labels=None):
    """EDMPrecond.forward with precondition=False and out_mul=2: (theta_pred [B,6,H,W], noise_pred [B,3,H,W])."""
    dt = next(v for v in sd.values() if v.is_floating_point()).dtype
    x = x.to(dt)
    sigma = t.to(dt).reshape(-1, 1, 1, 1)
    c_in, c_noise = unet_ref.precond_coeffs(cfg["variant"], sigma)[4:6]
    if augment_labels is not None:
        augment_labels = augment_labels.to(dt)
    return unet_ref.dhariwal_unet(sd, cfg, c_in * x, c_noise.flatten(), augment_labels)


def _bc(t):
    return t.reshape(-1, 1, 1, 1)


def q_sample(x0, noise, t, K, C=None):
    K = K.clamp(-1.0, 1.0)
    if C is None:
        C = -1 * x0 - K / 2
    time = _bc(t)
    return x0 + K / 2 * time ** 2 + C * time + torch.sqrt(time) * noise


def x_rec(x_noisy, theta_pred, noise_pred, t):
    K_pred, C_pred = theta_pred.chunk(2, dim=1)
    time = _bc(t)
    return x_noisy - K_pred / 2 * time ** 2 - C_pred * time - torch.sqrt(time) * noise_pred


def loss_weights(t, eps, weighting_loss):
    if not weighting_loss:
        return torch.ones_like(t), torch.ones_like(t)
    return 1 / t, 1 / (1 - t + eps)


def vlb(per_sample, t):
    """[B] * [B,1]^2 -> [B,B], mean: the product of the two means."""
    return (per_sample * (1 - t.reshape(-1, 1)) ** 2).mean()


def losses(theta_pred, noise_pred, x0, noise, K, x_noisy, t, eps, weighting_loss, use_l1, lpips_fn=None):
    """(loss, log) of p_losses from the predictions.  lpips_fn(x_rec, x0) -> [B] or None."""
    K = K.clamp(-1.0, 1.0)
    C = -1 * x0 - K / 2
    target1 = torch.cat([K, C], dim=1)
    w1, w2 = loss_weights(t, eps, weighting_loss)
    simple = w1 * ((theta_pred - target1) ** 2).mean([1, 2, 3]) + w2 * ((noise_pred - noise) ** 2).mean([1, 2, 3])
    if use_l1:
        simple = simple + w1 * (theta_pred - target1).abs().mean([1, 2, 3]) + w2 * (noise_pred - noise).abs().mean([1, 2, 3])
        simple = simple / 2
    loss_simple = simple.mean()
    xr = x_rec(x_noisy, theta_pred, noise_pred, t)
    per = (xr - x0).abs().mean([1, 2, 3])
    if lpips_fn is not None:
        per = per + lpips_fn(xr, x0)
    loss_vlb = vlb(per, t)
    loss = loss_simple + loss_vlb
    return loss, {"train/loss_simple": loss_simple, "train/loss_vlb": loss_vlb, "train/loss": loss}


def p_losses(model_fn, x0, t, noise, K, eps, weighting_loss, use_l1, lpips_fn=None, **model_kw):
    """model_fn(x_noisy, t, **model_kw) -> (theta_pred, noise_pred).  Returns (loss, log, x_noisy)."""
    x_noisy = q_sample(x0, noise, t, K)
    theta_pred, noise_pred = model_fn(x_noisy, t, **model_kw)
    loss, log = losses(theta_pred, noise_pred, x0, noise, K, x_noisy, t, eps, weighting_loss, use_l1, lpips_fn)
    return loss, log, x_noisy


def sampler_step(x, theta_pred, noise_pred, z, t, s):
    K, C = theta_pred.chunk(2, dim=1)
    K = K.clamp(-1.0, 1.0)
    time, s = _bc(t), _bc(s)
    mean = x + K / 2 * s ** 2 - K * time * s - C * s - s / torch.sqrt(time) * noise_pred
    return mean + torch.sqrt(s * (time - s) / time) * z


def finish(x, scale_input=1.0):
    x = x.clamp(-1.0 * scale_input, 1.0 * scale_input)
    if scale_input != 1:
        x = x / scale_input
    return (x + 1) * 0.5


def time_grid(n, eps, denoise):
    """[(cur_time, s)] as fp32 0-dim tensors, in the reference's fp32 arithmetic."""
    steps = torch.tensor([1.0 / n]).repeat(n)
    if denoise:
        e = torch.tensor([eps], dtype=torch.float32)
        steps = torch.cat((steps[:-1], steps[-1:] - e, e))
    cur = torch.ones(())
    out = []
    for i in range(steps.shape[0]):
        s = cur if i == steps.shape[0] - 1 else steps[i]
        out.append((cur, s))
        cur = cur - s
    return out


def sample_fn(model_fn, x_T, epsilons, n, eps, denoise, scale_input=1.0, sigma_max=1.0):
    """Returns (image in [0,1], [state after every step, before the final clamp], [share of clamped K predictions per step]).
    The state has x_T's dtype; time enters as the fp32 grid's values."""
    x = x_T * sigma_max
    B = x.shape[0]
    traj, clamped = [], []
    for k, (cur, s) in enumerate(time_grid(n, eps, denoise)):
        t_vec, s_vec = cur.to(x.dtype).expand(B), s.to(x.dtype).expand(B)
        theta, noise = model_fn(x, t_vec)
        clamped.append(float((theta[:, :theta.shape[1] // 2].abs() > 1).double().mean()))
        x = sampler_step(x, theta.to(x.dtype), noise.to(x.dtype), epsilons[k].to(x.dtype), t_vec, s_vec)
        traj.append(x)
    return finish(x, scale_input), traj, clamped


# ---------------------------------------------------------------------------------------------------------------------------
# the fixed cases of tests/golden/g17_linear.npz (tools/make_golden_linear.py writes it, the host and GPU tests read it)
# ---------------------------------------------------------------------------------------------------------------------------
EPS = 1e-4
GRAD_HEAD = 1024          # leading entries stored of each gradient (its norm is stored whole)
GRAD_KEYS = ["model.map_layer0.weight", "model.enc.32x32_conv.weight", "model.enc.16x16_block0.qkv.weight",
             "model.dec.16x16_up.conv0.weight", "model.dec.32x32_block1.skip.weight", "model.dec2.8x8_block0.norm1.weight",
             "model.decouple1.1.map.weight", "model.out_norm.weight", "model.out_conv.weight", "model.out_conv.bias",
             "model.out_conv2.weight", "model.map_augment.weight"]
STEP_GRAD_KEYS = ["model.map_layer1.bias", "model.out_conv.weight", "model.out_conv2.weight", "model.enc.16x16_block0.conv1.weight"]
STEP_VARIANTS = [(w, l1) for w in (0, 1) for l1 in (0, 1)]        # (weighting_loss, use_l1)
SAMPLING_TIMESTEPS = 10


def unet_inputs():
    """(x [2,3,32,32], sigma [2], augment labels [2,9]) of the reduced-width UNet cases."""
    return fill.hash_tensor((2, 3, 32, 32), "lin.x", 1.0), torch.tensor([0.05, 0.7]), fill.hash_tensor((2, 9), "lin.aug", 1.0)


def unet_objective(theta_pred, noise_pred):
    """The scalar whose gradients the UNet cases store: fixed weights on both outputs."""
    wt = fill.hash_tensor(tuple(theta_pred.shape), "lin.gx", 1.0).to(theta_pred)
    wn = fill.hash_tensor(tuple(noise_pred.shape), "lin.gy", 1.0).to(noise_pred)
    return (theta_pred * wt).sum() + (noise_pred * wn).sum()


def unet_inputs_full():
    return fill.hash_tensor((1, 3, 32, 32), "lin.xf", 1.0), torch.tensor([0.31]), fill.hash_tensor((1, 9), "lin.augf", 1.0)


def step_inputs():
    """(x0, t, noise, K) of the training-step cases: t reaches eps and 0.999; half of K lies outside [-1, 1] before its clamp."""
    return (fill.hash_tensor((4, 3, 32, 32), "lin.x0", 1.0), torch.tensor([1e-4, 0.3, 0.7, 0.999]),
            fill.hash_tensor((4, 3, 32, 32), "lin.noise", 1.7), fill.hash_tensor((4, 3, 32, 32), "lin.K", 2.0))


def sampler_inputs():
    """(x_T, [11 draws]) of the sampler cases."""
    return fill.hash_tensor((2, 3, 32, 32), "lin.xT", 1.7), [fill.hash_tensor((2, 3, 32, 32), f"lin.z{k}", 1.7) for k in range(11)]


def small_unet_state():
    """(cfg, closed-form state dict) of the reduced-width out_mul = 2 UNet."""
    cfg, shapes = cfg_and_shapes(**SMALL)
    return cfg, fill.filled_state_dict(shapes)


def full_unet_state():
    cfg, shapes = cfg_and_shapes(**FULL)
    return cfg, fill.filled_state_dict(shapes)
