"""GPU: the linear-drift DDM (ddm.ddm_linear) on the HIP path, against tests/linear_ref.py in fp64 or the reference-made fixture
tests/golden/g17_linear.npz (tests/test_linear_host.py pins the former to the latter on the CPU).

Tolerances: tests/parity.py::close for tensors (rtol 1e-3 / atol 1e-4, scaled by the tensor's own maximum); 1e-3 relative for scalar
losses and 2e-3 relative L2 for whole gradients, the limits of tests/test_hip_lpips.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import linear_ref
import lpips_ref
from oracle import fill
from parity import close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAML = os.path.join(ROOT, "configs", "cifar10", "ddm_uncond_linear_uncond_unet.yaml")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip
    hip.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g17():
    return dict(np.load(os.path.join(GOLDEN, "g17_linear.npz")))


def rel_l2(got, want):
    got, want = torch.as_tensor(np.asarray(got.detach().cpu() if isinstance(got, torch.Tensor) else got)).double(), \
        torch.as_tensor(np.asarray(want.detach().cpu() if isinstance(want, torch.Tensor) else want)).double()
    return float((got - want).norm() / want.norm())


def scalar_close(got, want, what):
    got, want = (float(v.detach()) if isinstance(v, torch.Tensor) else float(v) for v in (got, want))
    print(f"{what}: {got:.8g} (want {want:.8g}, rel {abs(got - want) / abs(want):.2e})")
    assert abs(got - want) <= 1e-3 * abs(want), (what, got, want)


def kernel_inputs(B=4, size=32):
    """x0 in [-1,1], noise, a K draw of which half lies outside [-1,1], t with eps and 0.999 in the batch, and predictions."""
    shape = (B, 3, size, size)
    x0 = fill.hash_tensor(shape, "lk.x0", 1.0)
    noise = fill.hash_tensor(shape, "lk.noise", 1.7)
    K = fill.hash_tensor(shape, "lk.K", 2.0)
    t = torch.tensor([1e-4, 0.999, 0.3, 0.62, 0.05, 0.9, 0.45, 0.77][:B])
    theta = fill.hash_tensor((B, 6, size, size), "lk.theta", 2.0)
    n_pred = fill.hash_tensor(shape, "lk.npred", 1.5)
    return x0, noise, K, t, theta, n_pred


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the kernels on their own
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [32, 5])          # 5: H W not a multiple of four -> the scalar form of the kernel
def test_q_sample_linear(gpu, size):
    from adm_amd import ops
    x0, noise, K, t, _, _ = kernel_inputs(size=size)
    assert 0.25 <= float((K.abs() > 1).double().mean()) <= 0.75
    got = ops.q_sample_linear(x0.to(gpu), noise.to(gpu), K.to(gpu), t.to(gpu))
    want = linear_ref.q_sample(x0.double(), noise.double(), t.double(), K.double())
    close(got, want)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(x0.shape)


@pytest.mark.parametrize("weighting,use_l1", linear_ref.STEP_VARIANTS)
@pytest.mark.parametrize("size", [32, 5])          # 5: the scalar form
def test_ddm_loss_linear(gpu, weighting, use_l1, size):
    from adm_amd import ops
    x0, noise, K, t, theta, n_pred = kernel_inputs(size=size)
    B = x0.shape[0]
    x_noisy = linear_ref.q_sample(x0, noise, t, K)
    th64, n64 = theta.double().requires_grad_(True), n_pred.double().requires_grad_(True)
    loss_r, log_r = linear_ref.losses(th64, n64, x0.double(), noise.double(), K.double(), x_noisy.double(), t.double(), linear_ref.EPS,
                                      bool(weighting), bool(use_l1))
    loss_r.backward()
    w1, w2 = linear_ref.loss_weights(t, linear_ref.EPS, bool(weighting))
    rec = ((1 - t) ** 2).mean()
    w = torch.stack([w1, w2, (rec / B).expand(B)], dim=1).contiguous()
    thd, nd = theta.to(gpu).requires_grad_(True), n_pred.to(gpu).requires_grad_(True)
    loss, per_simple, per_mae = ops.ddm_loss_linear(thd, nd, x0.to(gpu), noise.to(gpu), K.to(gpu), x_noisy.to(gpu), t.to(gpu), w.to(gpu),
                                                    bool(use_l1))
    loss.backward()
    torch.cuda.synchronize()
    tag = f"loss kernel w{weighting} l1{use_l1} {size}x{size}"
    scalar_close(loss, loss_r, tag + " loss")
    scalar_close(per_simple.sum() / B, log_r["train/loss_simple"], tag + " loss_simple")
    scalar_close(per_mae.sum() / B * rec.to(gpu), log_r["train/loss_vlb"], tag + " loss_vlb")
    close(thd.grad, th64.grad); close(nd.grad, n64.grad)
    for b in range(B):       # per image: under weighting_loss the image at t = eps carries nearly all of the norm
        e1, e2 = rel_l2(thd.grad[b], th64.grad[b]), rel_l2(nd.grad[b], n64.grad[b])
        print(f"{tag} image {b} (t = {float(t[b]):g}): d theta rel L2 {e1:.2e}, d noise rel L2 {e2:.2e}")
        assert e1 <= 2e-3 and e2 <= 2e-3


def test_lpips_input_linear_and_adjoint(gpu):
    from adm_amd import ops
    x0, noise, K, t, theta, n_pred = kernel_inputs()
    x_noisy = linear_ref.q_sample(x0, noise, t, K)
    shift, scale = torch.tensor([-.030, -.088, -.188]), torch.tensor([.458, .448, .450])
    th64, n64 = theta.double().requires_grad_(True), n_pred.double().requires_grad_(True)
    y_r = ((linear_ref.x_rec(x_noisy.double(), th64, n64, t.double()) - shift.double().reshape(1, 3, 1, 1)) / scale.double().reshape(1, 3, 1, 1))
    gy = fill.hash_tensor((4, 32, 32, 32), "lk.gy", 1.0)                # NHWC, all 32 channels: the padding's gradient must go nowhere
    (y_r * gy[..., :3].permute(0, 3, 1, 2).double()).sum().backward()
    thd, nd = theta.to(gpu).requires_grad_(True), n_pred.to(gpu).requires_grad_(True)
    y = ops.lpips_input(thd, nd, x_noisy.to(gpu), t.to(gpu), shift.to(gpu), scale.to(gpu), 2)
    assert tuple(y.shape) == (4, 32, 32, 32) and float(y[..., 3:].abs().max()) == 0.0
    (y * gy.to(gpu)).sum().backward()
    close(y[..., :3].permute(0, 3, 1, 2), y_r)
    close(thd.grad, th64.grad); close(nd.grad, n64.grad)
    assert rel_l2(thd.grad, th64.grad) <= 2e-3 and rel_l2(nd.grad, n64.grad) <= 2e-3
    with pytest.raises(NotImplementedError):
        ops.lpips_input(n_pred.to(gpu), nd, x_noisy.to(gpu), t.to(gpu), shift.to(gpu), scale.to(gpu), 2)     # three channels: not theta_pred


@pytest.mark.parametrize("last,scale_input", [(False, 1.0), (True, 1.0), (True, 2.0)])
def test_sampler_step_linear(gpu, last, scale_input):
    from adm_amd import ops
    B = 4
    x = fill.hash_tensor((B, 3, 32, 32), "ls.x", 1.5 * scale_input)
    theta = fill.hash_tensor((B, 6, 32, 32), "ls.theta", 2.0)         # K_pred ~ U(-2, 2): half of it is clamped
    outside = float((theta[:, :3].abs() > 1).double().mean())
    assert 0.25 <= outside <= 0.75, outside
    n_pred = fill.hash_tensor((B, 3, 32, 32), "ls.npred", 1.5)
    z = fill.hash_tensor((B, 3, 32, 32), "ls.z", 1.7)
    t = torch.tensor([1.0, 0.6, 0.1, 1e-4])
    s = torch.tensor([0.1, 0.1, 0.1 - 1e-4, 1e-4])                     # the last image: s = t, sigma exactly 0
    want = linear_ref.sampler_step(x.double(), theta.double(), n_pred.double(), z.double(), t.double(), s.double())
    Kp = theta[:, :3].double()
    moved = (Kp - Kp.clamp(-1, 1)) * (s ** 2 / 2 - t * s).double().reshape(-1, 1, 1, 1)
    assert float(moved.abs().max()) > 1e-2                             # (the clamp moves the result far more than the tolerance: the comparison sees it)
    if last:
        want = linear_ref.finish(want, scale_input)
    xd = x.to(gpu).clone()
    out = ops.sampler_step_linear(xd, theta.to(gpu), n_pred.to(gpu), z.to(gpu), t.to(gpu), s.to(gpu), scale_input, last)
    assert out.data_ptr() == xd.data_ptr() and out.dtype == torch.float32
    close(out, want)
    if last:
        assert 0.0 <= float(out.min()) and float(out.max()) <= 1.0
        sat = float(((out == 0) | (out == 1)).double().mean())
        assert 0.02 < sat < 0.98, sat            # both the clamped and the free range are compared


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the six-channel head at full width
# ---------------------------------------------------------------------------------------------------------------------------
def test_head_192_to_6_full_width(gpu, monkeypatch):
    from adm_amd import ops
    B, C, H = 8, 192, 32
    x = fill.hash_tensor((B, C, H, H), "lh.x", 1.5) + 0.2
    w = fill.hash_tensor((6, C, 3, 3), "lh.w", (1.0 / (C * 9)) ** 0.5)
    b = fill.hash_tensor((6,), "lh.b", 0.1)
    gamma, beta = 1 + fill.hash_tensor((C,), "lh.g", 0.2), fill.hash_tensor((C,), "lh.be", 0.1)
    gy = fill.hash_tensor((B, 6, H, H), "lh.gy", 1.0)
    xr, wr, br = (v.double().clone().requires_grad_(True) for v in (x, w, b))
    yr = F.conv2d(F.silu(F.group_norm(xr, 32, gamma.double(), beta.double())), wr, br, padding=1)
    (yr * gy.double()).sum().backward()

    def run():
        xd = x.permute(0, 2, 3, 1).contiguous().to(gpu).requires_grad_(True)
        wd, bd = w.to(gpu).requires_grad_(True), b.to(gpu).requires_grad_(True)
        h = ops.group_norm_act(xd, gamma.to(gpu), beta.to(gpu), None, silu=True, to_conv=True)      # as out_norm feeds out_conv in the UNet
        y = ops.head_out(ops.conv2d(h, wd, bd), 6)
        (y * gy.to(gpu)).sum().backward()
        torch.cuda.synchronize()
        return y.detach(), xd.grad, wd.grad, bd.grad

    regs, calls = [], []
    reg, call = ops._reg_amax, ops.call
    monkeypatch.setattr(ops, "_reg_amax", lambda t, slot: (regs.append((t, slot)), reg(t, slot))[1])
    monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append((name, a)), call(name, *a))[1])
    y, dx, dw, db = run()
    assert tuple(y.shape) == (B, 6, H, H)
    close(y, yr)
    close(dx.permute(0, 3, 1, 2), xr.grad); close(dw, wr.grad); close(db, br.grad)
    errs = dict(dx=rel_l2(dx.permute(0, 3, 1, 2), xr.grad), dw=rel_l2(dw, wr.grad), db=rel_l2(db, br.grad))
    print("192 -> 6 head, B = 8, 32x32, rel L2 against fp64:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 2e-3
    names = [n for n, _ in calls]
    assert names.count("adm_nhwc_to_nchw") == 1 and names.count("adm_nhwc_to_nchw_bwd_amax") == 1
    assert "adm_precond_out" not in names and "adm_precond_out_bwd_amax" not in names
    if ops.FP16X3 and ops.BF16X6 and ops.COMPUTE == "f32":
        # the adjoint wrote the bound of df and registered it: the head conv's gradients find it
        bwd_args = dict(calls)["adm_nhwc_to_nchw_bwd_amax"]
        assert bwd_args[3] is not None
        head = [(t, s) for t, s in regs if s is not None and tuple(t.shape) == (B, H, H, 32)]
        assert len(head) == 1
        df, slot = head[0]
        assert float(df[..., 6:].abs().max()) == 0.0
        assert float(slot.max()) == float(df.abs().max()) == float(gy.abs().max())
    # once more with every registered bound verified against its tensor: a missing or stale bound fails loudly
    monkeypatch.setattr(ops, "AMAX_CHECK", True)
    y2, dx2, dw2, _ = run()
    close(y2, yr); close(dx2.permute(0, 3, 1, 2), xr.grad); close(dw2, wr.grad)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the UNet against the fixture
# ---------------------------------------------------------------------------------------------------------------------------
def make_unet(gpu, full=False):
    from adm_amd.unet.uncond_unet import EDMPrecond
    cfg, sd = linear_ref.full_unet_state() if full else linear_ref.small_unet_state()
    keys = ("model_channels", "channel_mult", "channel_mult_emb", "num_blocks", "attn_resolutions", "dropout", "augment_dim")
    unet = EDMPrecond(img_resolution=32, img_channels=3, model_type="DhariwalUNet", out_mul=2, precondition=False, **{k: cfg[k] for k in keys})
    unet.load_state_dict(sd, strict=True)
    return unet.to(gpu).eval(), cfg, sd


def grads_close(g17, tag, keys, params, prefix=""):
    worst = 0.0
    for k in keys:
        g = params[prefix + k].grad
        close(g.reshape(-1)[:linear_ref.GRAD_HEAD], g17[f"{tag}.grad.{k}"], scale=float(g.abs().max()))
        e = rel_l2(g.reshape(-1)[:linear_ref.GRAD_HEAD], g17[f"{tag}.grad.{k}"])
        n = abs(float(g.double().norm()) - float(g17[f"{tag}.gradnorm.{k}"])) / float(g17[f"{tag}.gradnorm.{k}"])
        print(f"{tag} grad {k}: leading entries rel L2 {e:.2e}, norm rel {n:.2e}")
        assert e <= 2e-3 and n <= 1e-3, (tag, k, e, n)
        worst = max(worst, e)
    return worst


@pytest.mark.parametrize("use_aug", [0, 1])
def test_unet_small_vs_fixture(gpu, g17, use_aug):
    unet, _, _ = make_unet(gpu)
    x, sigma, aug = linear_ref.unet_inputs()
    xd = x.to(gpu).requires_grad_(True)
    theta, noise = unet(xd, sigma.to(gpu), **(dict(augment_labels=aug.to(gpu)) if use_aug else {}))
    assert tuple(theta.shape) == (2, 6, 32, 32) and tuple(noise.shape) == (2, 3, 32, 32)
    linear_ref.unet_objective(theta, noise).backward()
    tag = f"unet.small.aug{use_aug}"
    close(theta, g17[tag + ".theta_pred"]); close(noise, g17[tag + ".noise_pred"]); close(xd.grad, g17[tag + ".dL_dx"])
    assert rel_l2(xd.grad, g17[tag + ".dL_dx"]) <= 2e-3
    keys = [k for k in linear_ref.GRAD_KEYS if use_aug or "map_augment" not in k]
    grads_close(g17, tag, keys, dict(unet.named_parameters()))


def test_unet_full_width_vs_fixture(gpu, g17):
    unet, _, _ = make_unet(gpu, full=True)
    assert tuple(unet.model.out_conv.weight.shape) == (6, 192, 3, 3)
    x, sigma, aug = linear_ref.unet_inputs_full()
    with torch.no_grad():
        theta, noise = unet(x.to(gpu), sigma.to(gpu), augment_labels=aug.to(gpu))
    close(theta, g17["unet.full.theta_pred"]); close(noise, g17["unet.full.noise_pred"])


# ---------------------------------------------------------------------------------------------------------------------------
# 8. training_step
# ---------------------------------------------------------------------------------------------------------------------------
def make_ddpm(gpu, weighting=True, use_l1=False, lpips_sd=None, sampling_timesteps=10):
    import warnings
    from adm_amd.ddm.ddm_linear import DDPM
    unet, cfg, sd = make_unet(gpu)
    mcfg = dict(eps=linear_ref.EPS, sigma_max=1, sigma_min=0.01, weighting_loss=bool(weighting), use_augment=False)
    if lpips_sd is None:
        dpm = DDPM(model=unet, image_size=[32, 32], sampling_timesteps=sampling_timesteps, perceptual_weight=0.0, use_l1=bool(use_l1), cfg=mcfg)
    else:
        from adm_amd.ddm.lpips import LPIPS
        with pytest.warns(UserWarning, match="MAE part alone"):       # true at construction: the weights arrive on the next line
            dpm = DDPM(model=unet, image_size=[32, 32], sampling_timesteps=sampling_timesteps, perceptual_weight=1.0, use_l1=bool(use_l1),
                       cfg=mcfg)
        dpm.set_perceptual_loss(LPIPS.from_state_dict(lpips_sd))
    return dpm.to(gpu).eval(), cfg, sd


def step(dpm, gpu):
    x0, t, noise, K = linear_ref.step_inputs()
    return dpm.training_step({"image": x0.to(gpu)}, t=t.to(gpu), noise=noise.to(gpu), K=K.to(gpu))


@pytest.mark.parametrize("weighting,use_l1", linear_ref.STEP_VARIANTS)
def test_training_step_vs_fixture(gpu, g17, weighting, use_l1):
    dpm, _, _ = make_ddpm(gpu, weighting, use_l1)
    x0, t, noise, K = linear_ref.step_inputs()
    close(dpm.q_sample(x0.to(gpu), noise.to(gpu), t.to(gpu), K.to(gpu)), g17["step.x_noisy"])
    loss, log = step(dpm, gpu)
    loss.backward()
    torch.cuda.synchronize()
    tag = f"step.w{weighting}.l1{use_l1}"
    assert set(log) == {"train/loss_simple", "train/loss_vlb", "train/loss"}
    scalar_close(loss, g17[tag + ".loss"], tag + " loss")
    for k in log:
        scalar_close(log[k], g17[f"{tag}.log.{k}"], f"{tag} {k}")
    gn = torch.sqrt(sum(p.grad.double().pow(2).sum() for p in dpm.parameters() if p.grad is not None))
    scalar_close(gn, g17[tag + ".grad_norm"], tag + " gradient norm")
    grads_close(g17, tag, linear_ref.STEP_GRAD_KEYS, dict(dpm.named_parameters()), prefix="model.")


def test_training_step_with_lpips_vs_restatement(gpu, monkeypatch):
    from adm_amd import ops
    lp_sd = lpips_ref.synthetic_state_dict()
    lp64 = lpips_ref.cast(lp_sd, torch.float64)
    dpm, cfg, sd = make_ddpm(gpu, True, False, lp_sd)
    assert dpm.lpips_active
    x0, t, noise, K = linear_ref.step_inputs()
    # fp64 restatement: the full loss, and the reconstruction term (MAE + LPIPS) alone
    sdo = {k: (v.double() if v.is_floating_point() else v.clone()).requires_grad_(v.is_floating_point() and "resample" not in k) for k, v in sd.items()}
    mf = lambda a, b: linear_ref.unet(sdo, cfg, a, b)
    lp_fn = lambda a, b: lpips_ref.lpips(lp64, a, b)
    args = (x0.double(), t.double(), noise.double(), K.double(), linear_ref.EPS, True, False)
    loss_r, log_r, _ = linear_ref.p_losses(mf, *args, lpips_fn=lp_fn)
    loss_r.backward()
    g_full = {k: v.grad.clone() for k, v in sdo.items() if v.grad is not None}
    for v in sdo.values():
        v.grad = None
    _, log_v, _ = linear_ref.p_losses(mf, *args, lpips_fn=lp_fn)
    log_v["train/loss_vlb"].backward()
    g_vlb = {k: v.grad.clone() for k, v in sdo.items() if v.grad is not None}
    _, log_mae, _ = linear_ref.p_losses(mf, *args)
    assert float(log_r["train/loss_vlb"]) > 1.05 * float(log_mae["train/loss_vlb"])       # the LPIPS summand is a visible part of the term

    loss, log = step(dpm, gpu)
    loss.backward()
    torch.cuda.synchronize()
    scalar_close(loss, loss_r, "loss with LPIPS")
    for k in log:
        scalar_close(log[k], log_r[k], k + " with LPIPS")
    params = dict(dpm.named_parameters())
    names = [k for k in g_full if params["model." + k].grad is not None]
    full = rel_l2(torch.cat([params["model." + k].grad.reshape(-1).cpu() for k in names]), torch.cat([g_full[k].reshape(-1) for k in names]))
    print(f"full loss with LPIPS: gradient of all parameters rel L2 {full:.2e}")
    assert full <= 2e-3
    assert all(p.grad is None for p in dpm.perceptual_loss.parameters())
    # the reconstruction term alone through the UNet (the squared-error gradient is far larger and would hide a wrong one)
    dpm.zero_grad(set_to_none=True)
    xg, tg, ng, Kg = (v.to(gpu) for v in (x0, t, noise, K))
    x_noisy = dpm.q_sample(xg, ng, tg, Kg)
    theta, n_pred = dpm.model(x_noisy, tg)
    theta, theta_lp = ops.fanout(theta, 2)
    n_pred, n_lp = ops.fanout(n_pred, 2)
    B = 4
    rec = ((1 - tg) ** 2).mean()
    w = torch.stack([torch.zeros_like(tg), torch.zeros_like(tg), (rec / B).expand(B)], dim=1).contiguous()      # w1 = w2 = 0: the MAE term alone
    mae_loss, _, _ = ops.ddm_loss_linear(theta, n_pred, xg, ng, Kg, x_noisy, tg, w, False)
    vlb = mae_loss + dpm.perceptual_loss.from_predictions(theta_lp, n_lp, x_noisy, tg, xg, dpm._sched).sum() / B * rec
    vlb.backward()
    scalar_close(vlb, log_r["train/loss_vlb"], "reconstruction term (MAE + LPIPS) alone")
    for key in ("out_conv.weight", "out_conv2.weight", "enc.16x16_block0.conv1.weight"):
        e = rel_l2(params["model.model." + key].grad, g_vlb["model." + key])
        print(f"reconstruction term alone, gradient at {key}: rel L2 {e:.2e} (norm {float(g_vlb['model.' + key].norm()):.3e} against the full "
              f"loss's {float(g_full['model.' + key].norm()):.3e})")
        assert e <= 2e-3
    # and the whole step under AMAX_CHECK
    monkeypatch.setattr(ops, "AMAX_CHECK", True)
    dpm.zero_grad(set_to_none=True)
    loss2, _ = step(dpm, gpu)
    loss2.backward()
    torch.cuda.synchronize()
    assert abs(float(loss2) - float(loss)) <= 1e-6 * abs(float(loss))


def test_inactive_lpips_keeps_the_mae_term(gpu):
    from adm_amd.ddm.ddm_linear import DDPM
    unet, _, _ = make_unet(gpu)
    mcfg = dict(eps=linear_ref.EPS, sigma_max=1, sigma_min=0.01, weighting_loss=True, use_augment=False)
    with pytest.warns(UserWarning, match="MAE part alone"):
        dpm = DDPM(model=unet, image_size=[32, 32], perceptual_weight=1.0, cfg=mcfg).to(gpu).eval()
    assert not dpm.lpips_active
    loss, log = step(dpm, gpu)
    loss0, log0 = step(make_ddpm(gpu)[0], gpu)
    assert float(log["train/loss_vlb"]) > 0 and float(loss) == float(loss0) and float(log["train/loss_vlb"]) == float(log0["train/loss_vlb"])


# ---------------------------------------------------------------------------------------------------------------------------
# 9. the sampler
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("denoise", [True, False])
def test_sample_vs_fixture(gpu, g17, denoise):
    dpm, _, _ = make_ddpm(gpu)
    xT, epsilons = linear_ref.sampler_inputs()
    tag = f"sample.denoise{int(denoise)}"
    states = g17["sample.denoise1.states"] if denoise else np.concatenate([g17["sample.denoise1.states"][:9], g17[tag + ".states_from9"]])
    n = 11 if denoise else 10
    calls = []
    hook = dpm.model.register_forward_hook(lambda m, a, out: calls.append(tuple(a[1].shape)))
    img = dpm.sample(batch_size=2, denoise=denoise, x_T=xT.to(gpu), epsilons=[e.to(gpu) for e in epsilons])
    assert len(calls) == n and all(c == (2,) for c in calls)           # 11 network evaluations, each with cur_time [B]
    assert img.dtype == torch.float32 and tuple(img.shape) == (2, 3, 32, 32)
    assert float(img.min()) >= 0.0 and float(img.max()) <= 1.0
    calls.clear()
    img2, traj = dpm.sample_fn((2, 3, 32, 32), unnormalize=True, denoise=denoise, x_T=xT.to(gpu), epsilons=[e.to(gpu) for e in epsilons],
                               return_traj=True)
    hook.remove()
    assert len(traj) == n == states.shape[0] and torch.equal(img, img2)
    grid = dpm.time_grid(denoise)
    assert np.array_equal(np.array([c for c, _ in grid], dtype=np.float32), g17[tag + ".t"])
    assert np.array_equal(np.array([s for _, s in grid], dtype=np.float32), g17[tag + ".s"])
    for k, x in enumerate(traj):       # every state BEFORE the final clamp: the saturated half of the final pixels hides nothing
        close(x, states[k])
        print(f"{tag} state {k}: max abs err {float((x.cpu().double() - torch.as_tensor(states[k]).double()).abs().max()):.2e} "
              f"(max |state| {float(np.abs(states[k]).max()):.2f})")
    close(img, g17[tag + ".img"])


# ---------------------------------------------------------------------------------------------------------------------------
# 11. one fused launch each
# ---------------------------------------------------------------------------------------------------------------------------
def test_training_step_launches_each_new_kernel_once(gpu, monkeypatch):
    from adm_amd import ops
    dpm, _, _ = make_ddpm(gpu, True, False, lpips_ref.synthetic_state_dict())
    loss, _ = step(dpm, gpu)           # warm-up: weight packing is not part of the step
    loss.backward()
    dpm.zero_grad(set_to_none=True)
    names, schedules = [], []
    call = ops.call

    def recording(name, *a):
        names.append(name)
        if name == "adm_lpips_input":
            schedules.append(a[9])
        if name == "adm_lpips_input_bwd":
            schedules.append(("bwd", a[7]))
        return call(name, *a)

    monkeypatch.setattr(ops, "call", recording)
    loss, _ = step(dpm, gpu)
    loss.backward()
    torch.cuda.synchronize()
    for name in ("adm_q_sample_linear", "adm_ddm_loss_linear", "adm_nhwc_to_nchw", "adm_nhwc_to_nchw_bwd_amax"):
        assert names.count(name) == 1, (name, names.count(name))
    assert sorted(map(str, schedules)) == sorted(map(str, [2, -1, ("bwd", 2)])), schedules       # x_rec of the new schedule, the target image; one adjoint
    assert "adm_q_sample" not in names and "adm_ddm_loss" not in names and "adm_ddm_loss_latent" not in names


# ---------------------------------------------------------------------------------------------------------------------------
# 10. the command-line tools on the recipe (a child process each: collected late)
# ---------------------------------------------------------------------------------------------------------------------------
def test_cli_train_and_sample_linear_recipe(gpu, tmp_path):
    cfg = yaml.load(open(YAML), Loader=yaml.SafeLoader)
    assert cfg["model"]["class_name"] == "ddm.ddm_linear.DDPM"
    cfg["model"]["unet"].update(model_channels=64, num_blocks=1)
    cfg["data"]["batch_size"] = 8
    res = str(tmp_path / "run")
    cfg["trainer"].update(results_folder=res, train_num_steps=2, save_and_sample_every=2, log_freq=1, test_before=False,
                          ema_update_after_step=1, ema_update_every=1)
    cfg["sampler"].update(batch_size=4, sample_num=8, ckpt_path=os.path.join(res, "model-1.pt"), save_folder=os.path.join(res, "png"))
    path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_uncond_dpm.py"), "--cfg", path, "--max-steps", "2"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import math
    import re
    lines = re.findall(r"\[Train Step\] (\d+)/2: loss=(\S+) loss_simple=(\S+) .*grad_norm=(\S+) images/sec=", r.stdout)
    assert [int(l[0]) for l in lines] == [1, 2], r.stdout[-2000:]
    assert all(math.isfinite(float(v)) and float(v) > 0 for l in lines for v in l[1:]), lines
    ck = torch.load(os.path.join(res, "model-1.pt"), map_location="cpu", weights_only=True)
    assert ck["step"] == 2 and tuple(ck["model"]["model.model.out_conv.weight"].shape) == (6, 64, 3, 3)
    assert all(torch.isfinite(v).all() for v in ck["model"].values() if v.is_floating_point())
    assert os.path.exists(os.path.join(res, "sample-1.png"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sample_uncond.py"), "--cfg", path], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    names = sorted(os.listdir(os.path.join(res, "png")))
    assert names == [f"{i: 010d}.png" for i in range(8)], names
    from PIL import Image
    assert Image.open(os.path.join(res, "png", names[0])).size == (32, 32)
