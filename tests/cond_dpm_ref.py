"""Plain-PyTorch CPU restatement of the conditional PIXEL-SPACE training step (TEST INFRASTRUCTURE ONLY), in whatever dtype its
inputs have (the tests use fp64): DDPM.p_losses with use_l1 and a condition.

Restated from the reference: ddm/ddm_const_2.py:199-258 (p_losses; x_rec :217, weights :227-233, the SSE terms :235-236, the L1 twins
as per-sample MEANS :237-240, rec_weight and the LPIPS term :242-249, the loss and the three logged values :251-256) and
ddm/ddm_const.py:305-364 (the same with x_rec = -C_pred :326 and the weights of :336-338); training_step hands batch['cond'] on
positionally (ddm_const_2.py:157-161) and p_losses passes it to the model (:213).  The LPIPS term is tests/lpips_ref.py, whose
ScalingLayer broadcasts a one-channel image to three channels as the reference's does (taming/modules/losses/lpips.py:56-63).
tools/make_golden_cond_dpm.py checks this file against the imported reference and writes tests/golden/g24_cond_dpm.npz.
"""
import torch

import lpips_ref
from oracle import fill

EPS = 1e-4
SCHEDULES = ("const", "const_2")


def weights(schedule, t, eps, weighting_loss):
    if not weighting_loss:
        return torch.ones_like(t), torch.ones_like(t)
    if schedule == "const":                  # ddm_const.py:336-338
        return (t ** 2 - t + 1) / t, (t ** 2 - t + 1) / (1 - t + eps)
    return ((t - 1) / t) ** 2 + 1, (t / (1 - t + eps)) ** 2 + 1          # ddm_const_2.py:228-230


def q_sample(schedule, x0, noise, t):
    tt = t.reshape(-1, 1, 1, 1)
    return x0 + (-1 * x0) * tt + (tt.sqrt() if schedule == "const" else tt) * noise


def simple_terms(C_pred, noise_pred, x0, noise):
    """The four un-weighted per-sample terms: SSE_C, SSE_eps, mean|e_C|, mean|e_eps| (ddm_const_2.py:235-239)."""
    e1, e2 = C_pred - (-1 * x0), noise_pred - noise
    return (e1 ** 2).sum([1, 2, 3]), (e2 ** 2).sum([1, 2, 3]), e1.abs().mean([1, 2, 3]), e2.abs().mean([1, 2, 3])


def loss_simple(C_pred, noise_pred, x0, noise, w1, w2, use_l1=True):
    s1, s2, a1, a2 = simple_terms(C_pred, noise_pred, x0, noise)
    out = w1 * s1 + w2 * s2
    if use_l1:
        out = (out + w1 * a1 + w2 * a2) / 2
    return out


def ddm_loss_l1(c_pred, n_pred, x0, noise, w, gscale):
    """What adm_ddm_loss_l1 computes, in the dtype of its inputs: (per-sample loss_simple [B], dC_pred, dnoise_pred) with
    d = gscale * 0.5 * w * (2 e + sign(e) / n), sign(0) = 0."""
    n = c_pred[0].numel()
    per = loss_simple(c_pred, n_pred, x0, noise, w[:, 0], w[:, 1], True)
    e1, e2 = c_pred + x0, n_pred - noise
    k1, k2 = ((gscale * 0.5 * w[:, j]).reshape(-1, 1, 1, 1) for j in (0, 1))
    return per, k1 * (2 * e1 + torch.sign(e1) / n), k2 * (2 * e2 + torch.sign(e2) / n)


def losses(schedule, C_pred, noise_pred, x_noisy, x0, noise, t, eps, weighting_loss, use_l1=True, lpips_sd=None):
    """(loss, log, per-sample loss_simple) from the predictions.  lpips_sd None = perceptual_weight 0."""
    w1, w2 = weights(schedule, t, eps, weighting_loss)
    simple = loss_simple(C_pred, noise_pred, x0, noise, w1, w2, use_l1)
    B, n = x0.shape[0], x0[0].numel()
    if lpips_sd is not None:
        x_rec = lpips_ref.x_rec(schedule, C_pred, noise_pred, x_noisy, t)
        per = lpips_ref.lpips(lpips_ref.cast(lpips_sd, x0.dtype), x_rec, x0)
        vlb = lpips_ref.loss_vlb(per, t)          # the reference's [B] * [B,1] broadcast, / B
    else:
        vlb = torch.zeros((), dtype=x0.dtype)
    loss = simple.sum() / B + vlb
    log = {"train/loss_simple": simple.detach().sum() / B / n, "train/loss_vlb": vlb.detach() / n, "train/loss": loss.detach() / B / n}
    return loss, log, simple


def p_losses(schedule, model_fn, x0, t, noise, cond, eps, weighting_loss, use_l1=True, lpips_sd=None):
    """model_fn(x_noisy, t, cond) -> (C_pred, noise_pred)."""
    x_noisy = q_sample(schedule, x0, noise, t)
    C_pred, noise_pred = model_fn(x_noisy, t, cond)
    dt = x0.dtype if lpips_sd is None else torch.float64
    loss, log, simple = losses(schedule, C_pred.to(dt), noise_pred.to(dt), x_noisy.to(dt), x0.to(dt), noise.to(dt), t.to(dt), eps,
                               weighting_loss, use_l1, lpips_sd)
    return loss, log, (x_noisy, C_pred, noise_pred)


# ---------------------------------------------------------------------------------------------------------------------------
# fixed inputs
# ---------------------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = ((3, 1, 5, 7), (2, 1, 67, 61))          # n = 35: below one block and ragged; n = 4087: several strides of 256, ragged


def loss_inputs(shape):
    """(C_pred, noise_pred, x0, noise, t) in fp32; a few elements have exactly zero error (their L1 gradient is 0)."""
    tag = "x".join(map(str, shape))
    x0 = fill.hash_tensor(shape, f"cdpm.x0.{tag}", 1.0)
    noise = fill.hash_tensor(shape, f"cdpm.noise.{tag}", 1.7)
    c = -x0 + fill.hash_tensor(shape, f"cdpm.ec.{tag}", 0.6)
    e = noise + fill.hash_tensor(shape, f"cdpm.ee.{tag}", 0.8)
    cf, ef = c.reshape(shape[0], -1), e.reshape(shape[0], -1)
    cf[:, ::11] = -x0.reshape(shape[0], -1)[:, ::11]
    ef[:, 3::13] = noise.reshape(shape[0], -1)[:, 3::13]
    t = torch.tensor([0.23, 0.81, 0.5])[:shape[0]]
    return c, e, x0, noise, t


# golden step (tools/make_golden_cond_dpm.py): recorded predictions of a stub model at [2,1,16,16]
STEP_SHAPE = (2, 1, 16, 16)
STEP_VARIANTS = (0, 1)          # weighting_loss


def step_inputs():
    x0 = fill.hash_tensor(STEP_SHAPE, "cdpm.step.x0", 1.0)
    noise = fill.hash_tensor(STEP_SHAPE, "cdpm.step.noise", 1.7)
    cond = fill.hash_tensor((2, 3, 16, 16), "cdpm.step.cond", 1.0)
    c = -x0 + fill.hash_tensor(STEP_SHAPE, "cdpm.step.ec", 0.5)
    e = noise + fill.hash_tensor(STEP_SHAPE, "cdpm.step.ee", 0.7)
    return x0, noise, cond, c, e, torch.tensor([0.23, 0.81])


# one-channel LPIPS network cases (B, size, seed): chosen by tools/make_golden_cond_dpm.py so that the fp32 restatement alone stays
# within half of each bar of tests/test_hip_lpips.py (values 1e-3, gradient 2e-3 relative L2); the gaps are in the g24 report
LPIPS_C1_CASES = ((2, 16, 1), (2, 32, 1))


def lpips_c1_inputs(B, size, seed):
    """x0 in [-1, 1] and x_rec = x0 + 0.3 N(0, 1), fp32 [B,1,H,W]."""
    x0 = fill.hash_tensor((B, 1, size, size), f"cdpm.lpips.x0.{size}.{seed}", 1.0)
    g = torch.Generator().manual_seed(2000 + seed)
    return x0 + 0.3 * torch.randn(x0.shape, generator=g), x0
