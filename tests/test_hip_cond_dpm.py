"""GPU: the conditional pixel-space recipe (configs/saliency/duts_cond_ddm_const_dpm.yaml, train_cond_dpm.py) -- the loss kernel with
the mean-L1 twins and the one-channel LPIPS input kernels against fp64, the one-channel LPIPS network, unet.cond_unet.Unet at
channels = 1, one training step with a condition, sample(cond=...), the batch source at this recipe's source-to-target ratio, and both
drivers end to end on a small DUTS tree.

Bars.  Kernel level: tests/parity.close (rtol 1e-3, atol 1e-4 x scale).  Network and wrapper level: those of tests/test_hip_lpips.py
(values at rtol 1e-3, gradients at 2e-3 relative L2); the one-channel inputs are conditioned on the CPU first
(tools/make_golden_cond_dpm.py; tests/test_cond_dpm_host.py::test_report_is_all_ok holds the measured gaps to half of each bar).
The denoiser: the checks of tests/test_hip_saliency.py::test_denoiser_at_the_recipe_shape_family_vs_oracle.
"""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import cond_dpm_ref as R
import duts_data_ref as DR
import lpips_ref
from oracle import cond_unet_ref as C
from oracle import ddm_ref, fill
from parity import close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINS = [[8, 8], [4, 4], [2, 2], [1, 1]]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def rel_l2(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).norm() / want.norm())


# ---------------------------------------------------------------------------------------------------------------------------
# adm_ddm_loss_l1
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["ones", "const", "const_2"])
@pytest.mark.parametrize("shape", R.LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ddm_loss_l1_vs_fp64(gpu, shape, weights):
    from adm_amd import ops
    c, e, x0, noise, t = R.loss_inputs(shape)
    B = shape[0]
    w = torch.stack(R.weights("const" if weights == "ones" else weights, t, R.EPS, weights != "ones"), dim=1).contiguous()
    per_r, dc_r, dn_r = R.ddm_loss_l1(c.double(), e.double(), x0.double(), noise.double(), w.double(), 1.0 / B)
    cd, ed = c.to(gpu).requires_grad_(True), e.to(gpu).requires_grad_(True)
    loss, per = ops.ddm_loss_l1(cd, ed, x0.to(gpu), noise.to(gpu), w.to(gpu))
    loss.backward()
    print(f"{weights} {shape}: per-sample {per.tolist()} (fp64 {per_r.tolist()})")
    close(per, per_r)
    close(loss, per_r.sum() / B)
    close(cd.grad, dc_r); close(ed.grad, dn_r)
    zc, ze = (c + x0) == 0, (e - noise) == 0          # exactly zero error: sign(0) = 0, so the whole gradient is 0 there
    assert int(zc.sum()) > 0 and int(ze.sum()) > 0
    assert float(cd.grad.cpu()[zc].abs().max()) == 0.0 and float(ed.grad.cpu()[ze].abs().max()) == 0.0


def test_ddm_loss_l1_without_gradients(gpu):
    """dc = dn = NULL through the raw ABI, as adm_ddm_loss allows: the four fp64 sums alone, un-weighted."""
    from adm_amd.hip import call, ptr
    shape = R.LOSS_SHAPES[1]
    c, e, x0, noise, t = R.loss_inputs(shape)
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    w = torch.stack(R.weights("const", t, R.EPS, True), dim=1).contiguous().to(gpu)
    sums = torch.full((B, 4), 7.0, dtype=torch.float64, device=gpu)          # (the call zero-fills it)
    args = [v.to(gpu) for v in (c, e, x0, noise)]
    call("adm_ddm_loss_l1", *(ptr(v) for v in args), ptr(w), ptr(sums), None, None, 1.0 / B, B, n)
    s1, s2, a1, a2 = R.simple_terms(c.double(), e.double(), x0.double(), noise.double())
    want = torch.stack([s1, s2, a1 * n, a2 * n], dim=1)
    assert float(((sums.cpu() - want).abs() / want).max()) <= 1e-6          # fp64 sums of f32 terms: the terms' own roundings
    again = torch.empty_like(sums)
    call("adm_ddm_loss_l1", *(ptr(v) for v in args), ptr(w), ptr(again), None, None, 1.0 / B, B, n)
    assert torch.equal(sums, again)          # one workgroup per sample: bit-reproducible


# ---------------------------------------------------------------------------------------------------------------------------
# adm_lpips_input_c1 / _bwd
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(5, 7), (16, 16)], ids=["5x7", "16x16"])
@pytest.mark.parametrize("schedule", [-1, 0, 1], ids=["image", "const", "const_2"])
def test_lpips_input_c1(gpu, schedule, hw):
    from adm_amd import ops
    B, (H, W) = 2, hw
    a = fill.hash_tensor((B, 1, H, W), "c1.a", 1.2)
    n_pred = fill.hash_tensor((B, 1, H, W), "c1.n", 1.5)
    x_noisy = fill.hash_tensor((B, 1, H, W), "c1.xt", 2.0)
    t = torch.tensor([0.23, 0.81])
    gy = fill.hash_tensor((B, H, W, 32), "c1.gy", 1.0)           # (what arrives in the pad channels must be ignored)
    sd = lpips_ref.synthetic_state_dict()
    shift, scale = sd["scaling_layer.shift"].clone(), sd["scaling_layer.scale"].clone()
    ar, nr = a.double().requires_grad_(True), n_pred.double().requires_grad_(True)
    xr = ar if schedule < 0 else lpips_ref.x_rec("const" if schedule == 0 else "const_2", ar, nr, x_noisy.double(), t.double())
    yr = (xr - shift.double()) / scale.double()                  # [B,1,H,W] against [1,3,1,1]: the reference's broadcast
    assert tuple(yr.shape) == (B, 3, H, W)
    (yr * nchw(gy[..., :3]).double()).sum().backward()
    dev = lambda v: v.to(gpu)
    runs = []
    for _ in range(2):
        ad, nd = dev(a).requires_grad_(True), dev(n_pred).requires_grad_(True)
        y = ops.lpips_input(ad, nd, dev(x_noisy), dev(t), dev(shift), dev(scale), schedule)
        (y * dev(gy)).sum().backward()
        runs.append((y.detach(), ad.grad, nd.grad))
    y, da, dn = runs[0]
    assert tuple(y.shape) == (B, H, W, 32) and float(y[..., 3:].abs().max()) == 0
    # forward: bit for bit what the three-channel kernel makes of the expanded image (the same arithmetic per channel)
    ex = lambda v: dev(v).expand(-1, 3, -1, -1).contiguous()
    y3 = ops.lpips_input(ex(a), ex(n_pred), ex(x_noisy), dev(t), dev(shift), dev(scale), schedule)
    assert torch.equal(y, y3)
    close(nchw(y[..., :3]), yr)
    # backward: against fp64, and the same bits twice (a fixed-order sum, no atomics)
    assert tuple(da.shape) == (B, 1, H, W)
    close(da, ar.grad)
    if schedule == 1:
        close(dn, nr.grad)
    else:
        assert dn is None
    assert torch.equal(runs[1][1], da) and (dn is None or torch.equal(runs[1][2], dn)) and torch.equal(runs[1][0], y)


# ---------------------------------------------------------------------------------------------------------------------------
# the one-channel LPIPS network
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.LPIPS_C1_CASES, ids=lambda c: "B%d_%dx%d_seed%d" % (c[0], c[1], c[1], c[2]))
def test_lpips_network_one_channel_vs_fp64(gpu, case):
    from adm_amd.ddm.lpips import LPIPS
    sd = lpips_ref.synthetic_state_dict()
    x, x0 = R.lpips_c1_inputs(*case)
    per_r, g_r, _ = lpips_ref.value_and_grad(sd, x, x0, torch.float64)
    assert tuple(g_r.shape) == tuple(x.shape)
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
    assert tuple(per.shape) == (case[0],) and tuple(g.shape) == tuple(x.shape)
    assert rel <= 1e-3
    assert rel_l2(g, g_r) <= 2e-3
    assert torch.equal(per, per2) and torch.equal(g, g2)
    assert all(p.grad is None for p in m.parameters())


# ---------------------------------------------------------------------------------------------------------------------------
# the denoiser at channels = 1
# ---------------------------------------------------------------------------------------------------------------------------
def make_unet(gpu, **kw):
    cfg = C.default_cfg(dim=32, two_decoders=True, channels=1, window_sizes1=WINS, window_sizes2=WINS)
    mod = importlib.import_module("unet.cond_unet")
    m = mod.Unet(dim=32, dim_mults=cfg["dim_mults"], cond_dim=32, cond_dim_mults=(), channels=1, cond_in_dim=3, window_sizes1=WINS,
                 window_sizes2=WINS, fourier_scale=16, cfg={"cond_net": "swin", "cond_pe": False}, **kw)
    sd = C.filled_state_dict(cfg)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("init_conv_mask.") for k in missing)
    for mm in m.modules():
        if isinstance(mm, torch.nn.Dropout):
            mm.p = 0.0
    return m.to(gpu).eval(), cfg, sd


def oracle_params(sd):
    return {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k and k != "time_mlp.0.W" else v.clone())
            for k, v in sd.items()}


def test_denoiser_at_one_channel_vs_oracle(gpu):
    """dim 32 x (1, 2, 4, 4), windows 8 / 4 / 2 / 1, B = 1, a 64x64 one-channel image (maps 64 / 32 / 16 / 8) with the condition maps
    16 / 8 / 4 / 2 injected: the 129-channel stem padded to 160, final_conv / final_conv2 with ONE output channel, precond_out on a
    one-channel NCHW tensor.  Forward, input gradients and weight gradients against the CPU oracle."""
    m, cfg, sd = make_unet(gpu)
    assert tuple(m.init_conv[0].weight.shape) == (32, 129, 7, 7) and tuple(m.final_conv.weight.shape) == (1, 32, 1, 1)
    x = fill.hash_tensor((1, 1, 64, 64), "cdpm.x", 1.0)
    tt = torch.tensor([0.4])
    hm = C.cond_features(1, 64, 64, tag="cdpm.t.hm")
    assert [tuple(h.shape[2:]) for h in hm] == [(16, 16), (8, 8), (4, 4), (2, 2)]
    gx, gy = fill.hash_tensor((1, 1, 64, 64), "cdpm.gx", 1.0), fill.hash_tensor((1, 1, 64, 64), "cdpm.gy", 1.0)
    xg = x.to(gpu).requires_grad_(True)
    hg = [h.to(gpu).requires_grad_(True) for h in hm]
    y1, y2 = m(xg, tt.to(gpu), hg)
    assert tuple(y1.shape) == (1, 1, 64, 64) and tuple(y2.shape) == (1, 1, 64, 64)
    sdo = oracle_params(sd)
    xo, ho = x.clone().requires_grad_(True), [h.clone().requires_grad_(True) for h in hm]
    o1, o2 = C.unet_forward(sdo, cfg, xo, tt, ho)
    close(y1, o1.detach()); close(y2, o2.detach())
    ((y1 * gx.to(gpu)).sum() + (y2 * gy.to(gpu)).sum()).backward()
    ((o1 * gx).sum() + (o2 * gy).sum()).backward()
    close(xg.grad, xo.grad)
    for got, want in zip(hg, ho):
        close(got.grad, want.grad)
    gmax = max(float(v.grad.double().norm()) for v in sdo.values() if v.requires_grad and v.grad is not None)
    named = {n: p for n, p in m.named_parameters() if p.requires_grad}
    bad = []
    for name, p in named.items():
        want = sdo[name].grad
        err = float((p.grad.cpu().double() - want.double()).norm() / (want.double().norm() + 1e-4 * gmax))
        if err > 2e-3:
            bad.append((name, err))
    assert not bad, bad[:10]
    names = list(named)
    for name in (names[0], names[len(names) // 4], names[len(names) // 2], names[3 * len(names) // 4], names[-1], "final_conv.weight",
                 "final_conv2.weight"):
        want = sdo[name].grad
        close(named[name].grad, want, scale=max(float(want.double().norm()) / 8, 1e-12))


# ---------------------------------------------------------------------------------------------------------------------------
# the wrapper: one training step with a condition; sample(cond=...)
# ---------------------------------------------------------------------------------------------------------------------------
GRAD_KEY = "downs.0.0.block1.proj.weight"


def make_dpm(gpu, schedule, lpips_sd=None, steps=3, sample_type="deterministic", unet_kw=None):
    m, cfg, sd = make_unet(gpu, **(unet_kw or {}))
    D = importlib.import_module("adm_amd.ddm.ddm_" + schedule).DDPM
    mcfg = dict(eps=R.EPS, sigma_max=1, sigma_min=0.01, weighting_loss=True, use_augment=False, sample_type=sample_type)
    build = lambda pw: D(model=m, image_size=[32, 32], sampling_timesteps=steps, loss_type="l2", start_dist="normal",
                         perceptual_weight=pw, use_l1=True, cfg=dict(mcfg))
    if lpips_sd is not None:
        from adm_amd.ddm.lpips import LPIPS
        with pytest.warns(UserWarning, match="loss_vlb is 0"):       # true at construction: the weights arrive on the next line
            dpm = build(1.0)
        dpm.set_perceptual_loss(LPIPS.from_state_dict(lpips_sd))
    else:
        dpm = build(0.0)
    return dpm.to(gpu).eval(), cfg, sd


def step_inputs():
    x0 = fill.hash_tensor((2, 1, 32, 32), "cdpm.w.x0", 1.0)
    noise = fill.hash_tensor((2, 1, 32, 32), "cdpm.w.noise", 1.7)
    hm = C.cond_features(2, 32, 32, tag="cdpm.w.hm")          # maps 32 / 16 / 8 / 4, condition maps 8 / 4 / 2 / 1
    return x0, noise, hm, torch.tensor([0.23, 0.81])


@pytest.mark.parametrize("schedule,lpips", [("const", True), ("const", False), ("const_2", True)],
                         ids=["const-lpips", "const-no_lpips", "const_2-lpips"])
def test_training_step_with_cond_vs_oracle(gpu, schedule, lpips):
    lp_sd = lpips_ref.synthetic_state_dict() if lpips else None
    dpm, cfg, sd = make_dpm(gpu, schedule, lp_sd)
    assert dpm.use_l1 and dpm.weighting_loss and dpm.lpips_active == lpips and dpm.channels == 1
    x0, noise, hm, t = step_inputs()
    batch = {"image": x0.to(gpu), "cond": [h.to(gpu) for h in hm]}
    loss, log = dpm.training_step(batch, t=t.to(gpu), noise=noise.to(gpu))
    loss.backward()
    torch.cuda.synchronize()
    sdo = oracle_params(sd)
    seen = []

    def mf(x, tt, cond):
        seen.append(cond)
        return C.unet_forward(sdo, cfg, x, tt, cond)

    loss_o, log_o, _ = R.p_losses(schedule, mf, x0, t, noise, hm, R.EPS, True, True, lp_sd)
    loss_o.backward()
    assert len(seen) == 1 and seen[0] is hm
    assert set(log) == {"train/loss_simple", "train/loss_vlb", "train/loss"}
    got = {"loss": float(loss), **{k: float(v) for k, v in log.items()}}
    want = {"loss": float(loss_o), **{k: float(v) for k, v in log_o.items()}}
    for k, v in got.items():
        print(f"{schedule} lpips={lpips} {k}: {v:.8g} (oracle {want[k]:.8g})")
        if k == "train/loss_vlb" and not lpips:
            assert v == 0.0 and want[k] == 0.0
        else:
            assert abs(v - want[k]) <= 1e-3 * abs(want[k]), (k, v, want[k])
    if lpips:
        assert got["train/loss_vlb"] > 0
    params = dict(dpm.model.named_parameters())
    names = [k for k, v in sdo.items() if v.requires_grad and v.grad is not None and params[k].grad is not None]
    assert len(names) > 700 and GRAD_KEY in names
    full = rel_l2(torch.cat([params[k].grad.reshape(-1).cpu() for k in names]), torch.cat([sdo[k].grad.reshape(-1) for k in names]))
    key = rel_l2(params[GRAD_KEY].grad, sdo[GRAD_KEY].grad)
    print(f"{schedule} lpips={lpips} gradient rel L2: all parameters {full:.2e}, {GRAD_KEY} {key:.2e}")
    assert full <= 2e-3 and key <= 2e-3
    if not lpips:
        return
    assert all(p.grad is None for p in dpm.perceptual_loss.parameters())
    # The LPIPS term alone: the SSE gradient is four orders of magnitude larger and would hide a wrong one.  It is checked AT the
    # wrapper's own predictions (the restatement is given the same C_pred / noise_pred / x_noisy), not through the denoiser: on
    # grey 32x32 inputs one ReLU or pool choice of VGG16 carries 0.4 % of this gradient, and the denoiser's outputs differ from the
    # CPU oracle's by up to 1e-5 -- measured on the CPU oracle, adding 1e-6 ... 3e-5 N(0, 1) to C_pred moved the LPIPS-only weight
    # gradients by 2.6e-3 ... 2.2e-2 relative L2 on every one of seven input sets tried, while fp32 against fp64 at the SAME
    # predictions stays at 1.5e-6.  The denoiser's backward is linear in what arrives here and is held by the checks above.
    xd, nd, td = x0.to(gpu), noise.to(gpu), t.to(gpu)
    with torch.no_grad():
        x_noisy = dpm.q_sample(xd, nd, td)
        C_pred, noise_pred = dpm.model(x_noisy, td, batch["cond"])
    Cd, Nd = C_pred.clone().requires_grad_(True), noise_pred.clone().requires_grad_(True)
    per = dpm.perceptual_loss.from_predictions(Cd, Nd, x_noisy, td, xd, dpm._sched)
    vlb = per.sum() * ((-torch.log(td) / 2).sum() / x0.shape[0])
    vlb.backward()
    Co, No = Cd.detach().cpu().double().requires_grad_(True), Nd.detach().cpu().double().requires_grad_(True)
    xr_o = lpips_ref.x_rec(schedule, Co, No, x_noisy.cpu().double(), t.double())
    vlb_o = lpips_ref.loss_vlb(lpips_ref.lpips(lpips_ref.cast(lp_sd, torch.float64), xr_o, x0.double()), t.double())
    vlb_o.backward()
    alone = rel_l2(Cd.grad, Co.grad)
    print(f"{schedule} LPIPS term alone: {float(vlb):.8g} (fp64 {float(vlb_o):.8g}); d/dC_pred rel L2 {alone:.2e} "
          f"(norm {float(Co.grad.norm()):.3e})")
    assert abs(float(vlb) - float(vlb_o)) <= 1e-3 * float(vlb_o)
    assert abs(float(vlb) / x0[0].numel() - got["train/loss_vlb"]) <= 1e-5 * got["train/loss_vlb"]      # what the step logged
    assert alone <= 2e-3
    if schedule == "const":          # x_rec = -C_pred: noise_pred takes no part
        assert Nd.grad is None and No.grad is None
    else:
        assert rel_l2(Nd.grad, No.grad) <= 2e-3


@pytest.mark.parametrize("sample_type", ["deterministic", "stochastic"])
def test_sample_with_cond_vs_oracle(gpu, sample_type):
    """3 steps, B = 2, injected x_T (and epsilons), the condition given as its four feature maps: against the oracle's sampler driven
    by the oracle denoiser.  Pixel-space 'const' keeps its x0 clamp."""
    dpm, cfg, sd = make_dpm(gpu, "const", steps=3, sample_type=sample_type)
    _, _, hm, _ = step_inputs()
    xT = fill.hash_tensor((2, 1, 32, 32), "cdpm.s.xT", 1.7, torch.float64)
    eps = [fill.hash_tensor((2, 1, 32, 32), f"cdpm.s.eps{k}", 1.7, torch.float64) for k in range(3)]
    img = dpm.sample(cond=[h.to(gpu) for h in hm], x_T=xT.to(gpu), epsilons=[e.to(gpu) for e in eps])
    assert tuple(img.shape) == (2, 1, 32, 32) and float(img.min()) >= 0 and float(img.max()) <= 1
    mf = lambda x, tt: C.unet_forward(sd, cfg, x, tt, hm)
    with torch.no_grad():
        if sample_type == "deterministic":
            want = ddm_ref.sample_fn_d("const", mf, xT, 3, 0.01, 1.0)
        else:
            want = ddm_ref.sample_fn_s("const", mf, xT, eps, 3, 0.01, 1.0)
    close(img, want)


def test_sample_encodes_the_condition_once(gpu):
    """With the built-in encoder in eval mode sample(cond=photo) runs it once and hands the features on; the per-step call
    (sample_fn_d given the photo) gives the same bits.  In train mode the per-step call stays."""
    torch.manual_seed(3)
    dpm, _, _ = make_dpm(gpu, "const", steps=3, unet_kw=dict(cond_encoder="swin_b"))
    enc = dpm.model.init_conv_mask
    calls = []
    hook = enc.register_forward_hook(lambda *a: calls.append(1))
    photo = fill.hash_tensor((2, 3, 32, 32), "cdpm.s.photo", 1.0).to(gpu)
    xT = fill.hash_tensor((2, 1, 32, 32), "cdpm.s.xT", 1.7, torch.float64).to(gpu)
    once = dpm.sample(cond=photo, x_T=xT)
    assert len(calls) == 1
    per_step = dpm.sample_fn_d((2, 1, 32, 32), x_T=xT, cond=photo)
    assert len(calls) == 1 + 3
    assert torch.equal(once, per_step)
    dpm.train()
    del calls[:]
    dpm.sample(cond=photo, x_T=xT)
    assert len(calls) == 3
    hook.remove()


# ---------------------------------------------------------------------------------------------------------------------------
# a small DUTS tree; the batch source at this recipe's ratio
# ---------------------------------------------------------------------------------------------------------------------------
SIZES = [((205, 170), (205, 170)), ((150, 210), (150, 210)), ((64, 64), (64, 64)), ((180, 200), (170, 210)), ((90, 120), (90, 120)),
         ((200, 140), (200, 140))]


def duts_tree(root):
    """Six ragged pairs written with PIL, four under DUTS-TR and two under DUTS-TE; returns them as decoded back (jpg is lossy)."""
    from PIL import Image
    back = {}
    for split_dir, ids in (("DUTS-TR", range(4)), ("DUTS-TE", range(4, 6))):
        img_dir, mask_dir = root / split_dir / f"{split_dir}-Image", root / split_dir / f"{split_dir}-Mask"
        img_dir.mkdir(parents=True), mask_dir.mkdir(parents=True)
        back[split_dir] = []
        for i in ids:
            (ph, pw), (mh, mw) = SIZES[i]
            Image.fromarray(DR.hash_bytes((ph, pw, 3), f"cdpm.tree.p{i}")).save(img_dir / f"img_{i}.jpg", quality=90)
            Image.fromarray(DR.hash_bytes((mh, mw), f"cdpm.tree.m{i}")).save(mask_dir / f"img_{i}.png")
            back[split_dir].append((np.asarray(Image.open(img_dir / f"img_{i}.jpg").convert("RGB")),
                                    np.asarray(Image.open(mask_dir / f"img_{i}.png").convert("L"))))
    return back


def test_batch_source_at_ratio_3_2(gpu, tmp_path):
    """DUTSBatchStream at 64x64 from photos of 205x170 and 150x210 (ratios 3.2 / 2.7 and 2.3 / 3.3; the recipe resizes DUTS photos of
    about 400 px to 128), one map of another size than its photo: bit for bit against tests/duts_data_ref.py, which
    tests/test_duts_data_host.py pins to PIL's own bytes."""
    from adm_amd.ddm.pair_data import DUTSBatchStream
    back = duts_tree(tmp_path / "duts")["DUTS-TR"]
    assert back[0][0].shape[:2] == (205, 170) and back[1][0].shape[:2] == (150, 210) and back[3][1].shape != back[3][0].shape[:2]
    stream = DUTSBatchStream({"class_name": "ddm.data.DUTSDataset", "data_root": str(tmp_path / "duts"), "split": "train",
                              "augment_horizontal_flip": True}, 4, (64, 64), gpu, seed=5)
    idx, flip = [1, 0, 3, 0], [1, 0, 0, 1]
    batch = stream.next_batch(idx=idx, flip=flip, want_u8=True)
    want = [DR.duts_pair(*back[i], (64, 64), flip=bool(f)) for i, f in zip(idx, flip)]
    want_rgb, want_gray = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    assert list(batch)[:2] == ["image", "cond"]
    assert torch.equal(batch["cond_u8"].cpu(), torch.from_numpy(want_rgb)) and torch.equal(batch["image_u8"].cpu(), torch.from_numpy(want_gray))
    assert torch.equal(batch["cond"].cpu(), DR.to_float(want_rgb)) and torch.equal(batch["image"].cpu(), DR.gray_to_float(want_gray))
    assert tuple(batch["image"].shape) == (4, 1, 64, 64) and tuple(batch["cond"].shape) == (4, 3, 64, 64)


# ---------------------------------------------------------------------------------------------------------------------------
# the drivers
# ---------------------------------------------------------------------------------------------------------------------------
def reduced_cfg(tmp_path):
    cfg = yaml.load(open(os.path.join(ROOT, "configs/saliency/duts_cond_ddm_const_dpm_sample.yaml")), Loader=yaml.SafeLoader)
    cfg["model"].update(image_size=[64, 64], sampling_timesteps=2)
    cfg["model"]["unet"].update(dim=32)
    cfg["data"].update(class_name="ddm.data.DUTSDataset", data_root=str(tmp_path / "duts"), split="train", image_size=[64, 64],
                       batch_size=2, augment_horizontal_flip=True)
    res = str(tmp_path / "run")
    cfg["trainer"].update(results_folder=res, gradient_accumulate_every=2, train_num_steps=3, save_and_sample_every=2, log_freq=1,
                          test_before=True, ema_update_after_step=1, ema_update_every=1, resume_milestone=0)
    cfg["sampler"].update(sample_num=2, batch_size=2, use_ema=True, ckpt_path=os.path.join(res, "model-1.pt"),
                          save_folder=os.path.join(res, "png"))
    return cfg, res


def test_train_and_sample_cli_end_to_end(gpu, tmp_path):
    from PIL import Image
    duts_tree(tmp_path / "duts")
    cfg, res = reduced_cfg(tmp_path)
    path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "train_cond_dpm.py"), "--cfg", path,
                        "--max-steps", "2"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = [float(v) for v in re.findall(r"\[Train Step\] \d+/3: loss=(\S+)", r.stdout)]
    assert len(losses) == 2 and all(np.isfinite(losses)), r.stdout[-2000:]
    assert "DUTS pool: 4 pairs" in r.stdout
    ck = torch.load(os.path.join(res, "model-1.pt"), map_location="cpu", weights_only=True)
    assert ck["step"] == 2 and len([k for k in ck["model"] if k.startswith("model.init_conv_mask.features.")]) > 300
    assert tuple(ck["model"]["model.final_conv.weight"].shape) == (1, 32, 1, 1)
    for name in ("sample-0_2.png", "sample-1.png"):          # B = 2: one column, two rows; one channel
        im = Image.open(os.path.join(res, name))
        assert im.mode == "L" and im.size == (64, 128), (name, im.mode, im.size)
    # the sampler on that checkpoint: DUTS-TE in order, one mode-L prediction per photo under its name, PSNR against the resized map
    cfg["data"].update(split="test", augment_horizontal_flip=False)
    yaml.safe_dump(cfg, open(path, "w"))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "sample_cond_dpm.py"), "--cfg", path],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    psnr = re.search(r"PSNR: (-?\d+\.\d+)", r.stdout)
    assert psnr and np.isfinite(float(psnr.group(1))), r.stdout[-1000:]
    names = sorted(os.listdir(os.path.join(res, "png")))
    assert names == ["img_4.png", "img_5.png"], names
    for n in names:
        im = Image.open(os.path.join(res, "png", n))
        assert im.mode == "L" and im.size == (64, 64), (n, im.mode, im.size)
