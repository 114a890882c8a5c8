"""GPU parity of the LPIPS term: the kernels of csrc/lpips.hip one by one at the elementwise bar, the whole network and the
wrapper's training step against the fp64 restatement of tests/lpips_ref.py (synthetic VGG16 weights, the real lin weights).

Bars.  Kernel level: tests/parity.close (rtol 1e-3, atol 1e-4 x scale).  Network and wrapper level: values at rtol 1e-3, gradients
at 2e-3 relative L2 -- smoke()'s gradient bar, a norm on purpose: a near-zero pre-activation can flip one ReLU or one pool choice
between two correct fp32 implementations; tests/test_lpips_host.py checks on the CPU that torch's own fp32 stays within 2e-4 of
fp64 on these very inputs.  The head's gradient is also held to 1e-4 relative L2: it is at most 512-term fp32 sums of
well-separated values, whose rounding error is a few 1e-6, and the elementwise bar's absolute term alone would pass a gradient of
this size (it carries a 1 / HW) whatever its value.
"""
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

import lpips_ref
from oracle import fill
from parity import close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def rel_l2(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).norm() / want.norm())


# ---------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["distinct", "ties"])
@pytest.mark.parametrize("shape", [(2, 64, 8, 8), (3, 128, 4, 12), (1, 512, 2, 2)], ids=lambda s: "x".join(map(str, s)))
def test_maxpool2x2(gpu, kind, shape):
    from adm_amd import ops
    B, C, H, W = shape
    n = B * C * H * W
    if kind == "distinct":      # a permutation: no two values of the tensor, let alone of a window, are equal
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(7)).double()
        x = (perm / n - 0.5).reshape(shape)
    else:                       # three levels only: most windows hold their maximum more than once; one window is constant
        x = torch.round(fill.hash_tensor(shape, "pool.ties", 1.49, torch.float64))
        x[0, :, 0:2, 0:2] = 1.0
    gy = fill.hash_tensor((B, C, H // 2, W // 2), "pool.gy", 1.0, torch.float64)
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 2, 2)
    (yr * gy).sum().backward()
    xd = nhwc(x.float()).to(gpu).requires_grad_(True)
    y = ops.maxpool2x2(xd)
    (y * nhwc(gy.float()).to(gpu)).sum().backward()
    close(nchw(y), yr)
    close(nchw(xd.grad), xr.grad)
    assert torch.equal(nchw(y).cpu(), yr.detach().float())                   # a selection: exact
    assert torch.equal(nchw(xd.grad).cpu(), xr.grad.float())                 # ... ties included: the first maximum takes it


@pytest.mark.parametrize("schedule", [-1, 0, 1], ids=["image", "const", "const_2"])
def test_input_kernel(gpu, schedule):
    from adm_amd import ops
    B, H, W = 3, 16, 32
    a = fill.hash_tensor((B, 3, H, W), "in.a", 1.2)
    n_pred = fill.hash_tensor((B, 3, H, W), "in.n", 1.5)
    x_noisy = fill.hash_tensor((B, 3, H, W), "in.xt", 2.0)
    t = torch.tensor([0.23, 0.81, 0.5])
    gy = fill.hash_tensor((B, H, W, 32), "in.gy", 1.0)           # (what arrives in the pad channels must be ignored)
    shift = lpips_ref.synthetic_state_dict()["scaling_layer.shift"].clone()
    scale = lpips_ref.synthetic_state_dict()["scaling_layer.scale"].clone()
    ar, nr = a.double().requires_grad_(True), n_pred.double().requires_grad_(True)
    xr = ar if schedule < 0 else lpips_ref.x_rec("const" if schedule == 0 else "const_2", ar, nr, x_noisy.double(), t.double())
    yr = (xr - shift.double()) / scale.double()
    (yr * nchw(gy[..., :3]).double()).sum().backward()
    ad, nd = a.to(gpu).requires_grad_(True), n_pred.to(gpu).requires_grad_(True)
    y = ops.lpips_input(ad, nd, x_noisy.to(gpu), t.to(gpu), shift.to(gpu), scale.to(gpu), schedule)
    assert tuple(y.shape) == (B, H, W, 32) and float(y.detach()[..., 3:].abs().max()) == 0
    (y * gy.to(gpu)).sum().backward()
    close(nchw(y[..., :3]), yr)
    close(ad.grad, ar.grad)
    if schedule == 1:
        close(nd.grad, nr.grad)
    else:
        assert nd.grad is None


@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_head(gpu, C):
    from adm_amd import ops
    B, H, W = 3, 12, 12          # HW = 144: two workgroups per image, the second one partly filled
    f0 = F.relu(fill.hash_tensor((B, C, H, W), f"head.f0.{C}", 1.0, torch.float64) + 0.3)
    f1 = F.relu(f0 + fill.hash_tensor((B, C, H, W), f"head.f1.{C}", 0.3, torch.float64))
    f0[1, :, 5, 7] = 0.0         # one all-zero position: the reference's gradient is NaN there, the kernel's is zero
    w = lpips_ref.lin_state_dict()[f"lin{(64, 128, 256, 512).index(C)}.model.1.weight"]
    dout = torch.tensor([1.0, -0.7, 0.4], dtype=torch.float64) * H * W
    fr = f0.clone().requires_grad_(True)
    per_r = lpips_ref.head(fr, f1, w.double())
    (per_r * dout).sum().backward()
    dead = torch.zeros(B, 1, H, W, dtype=torch.bool)
    dead[1, 0, 5, 7] = True
    assert bool(torch.isnan(fr.grad[1, :, 5, 7]).all()) and not bool(torch.isnan(fr.grad.masked_fill(dead, 0.0)).any())
    want = fr.grad.masked_fill(dead, 0.0)
    fd = nhwc(f0.float()).to(gpu).requires_grad_(True)
    per = ops.lpips_heads([fd], [nhwc(f1.float()).to(gpu)], [w.to(gpu)])
    (per * dout.float().to(gpu)).sum().backward()
    got = nchw(fd.grad).cpu()
    print(f"C={C}: per-sample {per.tolist()} (fp64 {per_r.tolist()}), gradient rel L2 {rel_l2(got, want):.2e}")
    close(per, per_r)
    close(got, want)
    assert bool(torch.isfinite(got).all()) and float(got[1, :, 5, 7].abs().max()) == 0
    assert float(((per.cpu().double() - per_r.detach()).abs() / per_r.detach().abs()).max()) <= 1e-4
    assert rel_l2(got, want) <= 1e-4


# ---------------------------------------------------------------------------------------------------------------------------
# the network
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lpips_ref.NETWORK_CASES, ids=lambda c: "B%d_%dx%d_seed%d" % (c[0], c[1], c[1], c[2]))
def test_network_vs_fp64(gpu, case):
    from adm_amd.ddm.lpips import LPIPS
    sd = lpips_ref.synthetic_state_dict()
    x, x0 = lpips_ref.network_inputs(*case)
    per_r, g_r, _ = lpips_ref.value_and_grad(sd, x, x0, torch.float64)
    m = LPIPS.from_state_dict(sd).to(gpu)
    runs = []
    for _ in range(2):
        xd = x.to(gpu).requires_grad_(True)
        per = m(xd, x0.to(gpu))
        per.sum().backward()
        runs.append((per.detach().cpu(), xd.grad.cpu()))
    (per, g), (per2, g2) = runs
    rel = float(((per.double() - per_r).abs() / per_r.abs()).max())
    print(f"{case}: per-sample {per.tolist()} (fp64 {per_r.tolist()}): rel {rel:.2e}; d/dx_rec rel L2 {rel_l2(g, g_r):.2e}")
    assert tuple(per.shape) == (case[0],)
    assert rel <= 1e-3
    assert rel_l2(g, g_r) <= 2e-3
    assert torch.equal(per, per2) and torch.equal(g, g2)          # fixed-order sums: bit-reproducible
    assert all(p.grad is None for p in m.parameters())


# ---------------------------------------------------------------------------------------------------------------------------
# the wrapper
# ---------------------------------------------------------------------------------------------------------------------------
def make_ddpm(schedule, gpu, lpips_sd=None, perceptual_weight=None, **kw):
    if perceptual_weight is None:
        perceptual_weight = 1.0 if lpips_sd is not None else 0.0
    variant, eps = lpips_ref.WRAPPER[schedule]
    cfg, sd = lpips_ref.small_unet(schedule)
    keys = ("model_channels", "channel_mult", "channel_mult_emb", "num_blocks", "attn_resolutions", "dropout", "augment_dim")
    unet = importlib.import_module("adm_amd.unet." + variant).EDMPrecond(img_resolution=32, img_channels=3, model_type="DhariwalUNet",
                                                                         **{k: cfg[k] for k in keys})
    unet.load_state_dict(sd, strict=True)
    D = importlib.import_module("adm_amd.ddm.ddm_" + schedule).DDPM
    build = lambda: D(model=unet, image_size=[32, 32], sampling_timesteps=2, perceptual_weight=perceptual_weight,
                      cfg=dict(eps=eps, sigma_max=1, sigma_min=0.01, weighting_loss=True), **kw)
    if lpips_sd is not None:
        from adm_amd.ddm.lpips import LPIPS
        with pytest.warns(UserWarning, match="loss_vlb is 0"):       # true at construction: the weights arrive on the next line
            dpm = build()
        dpm.set_perceptual_loss(LPIPS.from_state_dict(lpips_sd))
    else:
        dpm = build()
    return dpm.to(gpu).eval()


def step(dpm, gpu):
    x0, noise, t = lpips_ref.wrapper_inputs()
    return dpm.training_step({"image": x0.to(gpu)}, t=t.to(gpu), noise=noise.to(gpu))


@pytest.mark.parametrize("schedule", ["const", "const_2"])
def test_training_step_vs_oracle(gpu, schedule, monkeypatch):
    from adm_amd import ops
    sd = lpips_ref.synthetic_state_dict()
    ref = lpips_ref.oracle_step(schedule, sd)
    dpm = make_ddpm(schedule, gpu, sd)
    assert dpm.lpips_active
    loss, log = step(dpm, gpu)
    loss.backward()
    torch.cuda.synchronize()
    assert set(log) == {"train/loss_simple", "train/loss_vlb", "train/loss"}
    got = {"loss": float(loss), "log_loss_simple": float(log["train/loss_simple"]), "log_loss_vlb": float(log["train/loss_vlb"])}
    for k, v in got.items():
        want = float(ref[k])
        print(f"{schedule} {k}: {v:.8g} (oracle {want:.8g}, rel {abs(v - want) / abs(want):.2e})")
        assert abs(v - want) <= 1e-3 * abs(want), (k, v, want)
    assert float(log["train/loss_vlb"]) > 0
    # the full loss: every parameter's gradient, as one vector and at smoke()'s parameter (guards the fan-out sum of the predictions)
    params = dict(dpm.named_parameters())
    names = []
    for k, g in ref["grads"].items():
        if params["model." + k].grad is None:       # (a parameter the step does not reach: the oracle's gradient is zero there)
            assert float(g.abs().max()) == 0, k
        else:
            names.append(k)
    g_hip = torch.cat([params["model." + k].grad.reshape(-1).cpu() for k in names])
    g_ref = torch.cat([ref["grads"][k].reshape(-1) for k in names])
    full, key = rel_l2(g_hip, g_ref), rel_l2(params["model." + lpips_ref.GRAD_KEY].grad, ref["grads"][lpips_ref.GRAD_KEY])
    print(f"{schedule} full-loss gradient rel L2: all parameters {full:.2e}, {lpips_ref.GRAD_KEY} {key:.2e}")
    assert full <= 2e-3 and key <= 2e-3
    assert all(p.grad is None for p in dpm.perceptual_loss.parameters())
    # the LPIPS term alone, through the UNet: the SSE gradient is four orders of magnitude larger and would hide a wrong one
    dpm.zero_grad(set_to_none=True)
    x0, noise, t = (v.to(gpu) for v in lpips_ref.wrapper_inputs())
    x_noisy = dpm.q_sample(x0, noise, t)
    C_pred, noise_pred = dpm.model(x_noisy, t)
    per = dpm.perceptual_loss.from_predictions(C_pred, noise_pred, x_noisy, t, x0, dpm._sched)
    vlb = per.sum() * ((-torch.log(t) / 2).sum() / x0.shape[0])
    vlb.backward()
    alone = rel_l2(params["model." + lpips_ref.GRAD_KEY].grad, ref["g_vlb"])
    print(f"{schedule} LPIPS term alone: {float(vlb):.8g} (oracle {float(ref['vlb']):.8g}); gradient at {lpips_ref.GRAD_KEY}: "
          f"rel L2 {alone:.2e} (norm {float(ref['g_vlb'].norm()):.3e} against the full loss's {float(ref['grads'][lpips_ref.GRAD_KEY].norm()):.3e})")
    assert abs(float(vlb) - float(ref["vlb"])) <= 1e-3 * float(ref["vlb"])
    assert alone <= 2e-3
    # once more with every registered bound verified against its tensor: a stale bound fails loudly
    monkeypatch.setattr(ops, "AMAX_CHECK", True)
    dpm.zero_grad(set_to_none=True)
    loss2, _ = step(dpm, gpu)
    loss2.backward()
    torch.cuda.synchronize()
    assert abs(float(loss2) - float(loss)) <= 1e-6 * abs(float(loss))


def test_checkpoint_brings_its_own_vgg16(gpu, tmp_path):
    sd = lpips_ref.synthetic_state_dict()
    dpm = make_ddpm("const", gpu, sd)
    _, log = step(dpm, gpu)
    torch.save({"model": {k: v.cpu() for k, v in dpm.state_dict().items()}}, tmp_path / "model-1.pt")
    dpm2 = make_ddpm("const", gpu, None, perceptual_weight=1.0, ckpt_path=str(tmp_path / "model-1.pt"))
    assert dpm2.lpips_active and not any(p.requires_grad for p in dpm2.perceptual_loss.parameters())
    _, log2 = step(dpm2, gpu)
    a, b = float(log["train/loss_vlb"]), float(log2["train/loss_vlb"])
    assert a > 0 and abs(a - b) <= 1e-6 * a, (a, b)


def test_inactive_term_is_todays_behaviour(gpu):
    """perceptual_weight > 0 without weights: the warning, loss_vlb = 0 and the loss of perceptual_weight = 0, bit for bit."""
    with pytest.warns(UserWarning, match="loss_vlb is 0"):
        dpm = make_ddpm("const", gpu, None, perceptual_weight=1.0)
    assert dpm.perceptual_weight == 1.0 and not dpm.lpips_active
    loss, log = step(dpm, gpu)
    loss0, _ = step(make_ddpm("const", gpu), gpu)
    assert float(log["train/loss_vlb"]) == 0.0 and math.isfinite(float(loss)) and float(loss) == float(loss0)
