#!/usr/bin/env python3
"""Golden vectors of the linear-drift DDM (ddm.ddm_linear).  RUNS ONLY WHERE THE REFERENCE IS (default /root/reference, or $ADM_REFERENCE).

Imports the reference's own ``unet.uncond_unet`` and ``ddm.ddm_linear`` with the two import-time shims of tools/make_golden.py (an
'ADM' package alias and an empty 'torchvision' stub), runs them on closed-form inputs and weights (oracle/fill.py), checks the
plain-torch restatement tests/linear_ref.py against them, and writes

  tests/golden/g17_linear.npz                                expected outputs only (the inputs are closed-form)
  tests/golden/oracle_vs_reference_report_linear.json        restatement errors, the wrapper's state-dict key list, clamp shares

Draws inside the reference (noise, K, the sampler's x_T and epsilons) are injected by patching torch.randn / torch.randn_like for
the duration of the call, in call order.  The fixtures are data the reference produced; none of its source is copied.
Usage:  python tools/make_golden_linear.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ADM_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

adm = types.ModuleType("ADM"); adm.__path__ = [REF]; sys.modules["ADM"] = adm
tv = types.ModuleType("torchvision"); tv.models = types.ModuleType("torchvision.models")
tv.transforms = types.ModuleType("torchvision.transforms")
sys.modules["torchvision"] = tv; sys.modules["torchvision.models"] = tv.models
sys.modules["torchvision.transforms"] = tv.transforms

import importlib  # noqa: E402

import linear_ref  # noqa: E402
from oracle import fill  # noqa: E402

U = importlib.import_module("unet.uncond_unet")
DL = importlib.import_module("ddm.ddm_linear")

OUT = os.path.join(ROOT, "tests", "golden")
torch.manual_seed(0)
torch.set_num_threads(8)
report = {"torch": torch.__version__, "cases": []}
g = {}

GRAD_KEYS, STEP_GRAD_KEYS, GRAD_HEAD, EPS = linear_ref.GRAD_KEYS, linear_ref.STEP_GRAD_KEYS, linear_ref.GRAD_HEAD, linear_ref.EPS


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def check(name, got, want, tol=2e-5):
    e = rel_err(torch.as_tensor(got), torch.as_tensor(want))
    ok = e <= tol
    report["cases"].append(dict(case=name, max_rel_err=e, tol=tol, ok=bool(ok)))
    print(f"{'OK ' if ok else 'BAD'} {name}: rel_err={e:.3e}")
    assert ok, name


def build_ref_unet(over):
    cfg, shapes = linear_ref.cfg_and_shapes(**over)
    kw = {k: cfg[k] for k in ("model_channels", "channel_mult", "channel_mult_emb", "num_blocks", "attn_resolutions", "dropout",
                              "augment_dim")}
    m = U.EDMPrecond(img_resolution=32, img_channels=3, model_type="DhariwalUNet", precondition=False, out_mul=2, **kw)
    ref_sd = m.state_dict()
    assert list(ref_sd.keys()) == list(shapes.keys()), "state_dict names/order differ"
    for k, v in ref_sd.items():
        assert tuple(v.shape) == tuple(shapes[k]), (k, tuple(v.shape), shapes[k])
    sd = fill.filled_state_dict(shapes)
    m.load_state_dict(sd, strict=True)
    return m.eval(), sd, cfg


class patched_draws:
    """torch.randn / torch.randn_like return the given tensors, in call order."""

    def __init__(self, draws):
        self.it = iter(draws)

    def __enter__(self):
        self.saved = (torch.randn, torch.randn_like)
        torch.randn = lambda *a, **k: next(self.it).clone()
        torch.randn_like = lambda *a, **k: next(self.it).clone()

    def __exit__(self, *a):
        torch.randn, torch.randn_like = self.saved


# ------------------------------------------------------------------------------------------------ UNet, out_mul = 2, precondition = False
m, sd, cfg = build_ref_unet(linear_ref.SMALL)
x, sigma, aug = linear_ref.unet_inputs()
wsum = linear_ref.unet_objective
for use_aug in (0, 1):
    kw = dict(augment_labels=aug) if use_aug else {}
    xr = x.clone().requires_grad_(True)
    th_ref, n_ref = m(xr, sigma, **kw)
    assert tuple(th_ref.shape) == (2, 6, 32, 32) and tuple(n_ref.shape) == (2, 3, 32, 32)
    wsum(th_ref, n_ref).backward()
    sdo = {k: v.clone().requires_grad_(v.is_floating_point() and "resample" not in k) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    th_o, n_o = linear_ref.unet(sdo, cfg, xo, sigma, **kw)
    wsum(th_o, n_o).backward()
    tag = f"unet.small.aug{use_aug}"
    check(tag + "/theta_pred", th_o, th_ref); check(tag + "/noise_pred", n_o, n_ref)
    check(tag + "/dL_dx", xo.grad, xr.grad, 1e-4)
    named = dict(m.named_parameters())
    g[tag + ".theta_pred"], g[tag + ".noise_pred"] = th_ref.detach().numpy(), n_ref.detach().numpy()
    g[tag + ".dL_dx"] = xr.grad.numpy().copy()
    for k in GRAD_KEYS:
        if "map_augment" in k and not use_aug:
            continue
        check(tag + "/grad/" + k, sdo[k].grad, named[k].grad, 1e-4)
        g[f"{tag}.grad.{k}"] = named[k].grad.reshape(-1)[:GRAD_HEAD].numpy().copy()
        g[f"{tag}.gradnorm.{k}"] = np.array(float(named[k].grad.double().norm()))
    m.zero_grad()

mf, sdf, cfgf = build_ref_unet(linear_ref.FULL)
xf, sf, augf = linear_ref.unet_inputs_full()
with torch.no_grad():
    th_ref, n_ref = mf(xf, sf, augment_labels=augf)
    th_o, n_o = linear_ref.unet(sdf, cfgf, xf, sf, augment_labels=augf)
check("unet.full/theta_pred", th_o, th_ref); check("unet.full/noise_pred", n_o, n_ref)
g["unet.full.theta_pred"], g["unet.full.noise_pred"] = th_ref.numpy(), n_ref.numpy()
del mf, sdf

# ------------------------------------------------------------------------------------------------ training_step, four loss variants
x0, t, noise, Kdraw = linear_ref.step_inputs()
for weighting, use_l1 in linear_ref.STEP_VARIANTS:
    mcfg = dict(eps=EPS, sigma_max=1, sigma_min=0.01, weighting_loss=bool(weighting), use_augment=False)
    dpm = DL.DDPM(model=m, image_size=[32, 32], sampling_timesteps=10, loss_type="l2", start_dist="normal",
                  perceptual_weight=0.0, use_l1=bool(use_l1), cfg=dict(mcfg))
    if not weighting and not use_l1:
        report["state_dict_keys"] = list(dpm.state_dict().keys())
    dpm.zero_grad()
    captured = {}
    orig_q = dpm.q_sample
    dpm.q_sample = lambda **kw: captured.setdefault("x_noisy", orig_q(**kw))
    with patched_draws([noise, Kdraw]):
        loss_ref, log_ref = dpm.p_losses(x0, t)
    dpm.q_sample = orig_q
    loss_ref.backward()
    sdo = {k: v.clone().requires_grad_(v.is_floating_point() and "resample" not in k) for k, v in sd.items()}
    loss_o, log_o, xn_o = linear_ref.p_losses(lambda a, b: linear_ref.unet(sdo, cfg, a, b), x0, t, noise, Kdraw, EPS,
                                              bool(weighting), bool(use_l1))
    loss_o.backward()
    tag = f"step.w{weighting}.l1{use_l1}"
    check(tag + "/x_noisy", xn_o, captured["x_noisy"], 1e-6)
    check(tag + "/loss", loss_o, loss_ref)
    for k in log_ref:
        check(tag + "/" + k, log_o[k], log_ref[k])
    named = dict(dpm.named_parameters())
    gn_ref = torch.sqrt(sum(p.grad.double().pow(2).sum() for p in dpm.parameters() if p.grad is not None))
    gn_o = torch.sqrt(sum(v.grad.double().pow(2).sum() for v in sdo.values() if v.grad is not None))
    check(tag + "/grad_norm", gn_o, gn_ref, 1e-4)
    if "step.x_noisy" in g:         # x_noisy depends on the draws alone, not on the loss variant: stored once
        assert np.array_equal(g["step.x_noisy"], captured["x_noisy"].detach().numpy())
    g["step.x_noisy"] = captured["x_noisy"].detach().numpy()
    g[tag + ".loss"] = loss_ref.detach().numpy()
    for k in log_ref:
        g[f"{tag}.log.{k}"] = log_ref[k].detach().numpy()
    g[tag + ".grad_norm"] = gn_ref.numpy()
    for k in STEP_GRAD_KEYS:
        check(tag + "/grad/" + k, sdo[k].grad, named["model." + k].grad, 1e-4)
        g[f"{tag}.grad.{k}"] = named["model." + k].grad.reshape(-1)[:GRAD_HEAD].numpy().copy()
        g[f"{tag}.gradnorm.{k}"] = np.array(float(named["model." + k].grad.double().norm()))
m.zero_grad()

# ------------------------------------------------------------------------------------------------ sample_fn, denoise True / False
xT, epsilons = linear_ref.sampler_inputs()
mcfg = dict(eps=EPS, sigma_max=1, sigma_min=0.01, weighting_loss=True, use_augment=False)
report["sampler"] = {}
for denoise in (True, False):
    dpm = DL.DDPM(model=m, image_size=[32, 32], sampling_timesteps=10, loss_type="l2", start_dist="normal",
                  perceptual_weight=0.0, cfg=dict(mcfg))
    rec = dict(t=[], s=[], x=[], kshare=[])
    orig = dpm.pred_xtms_from_xt

    def recording(xt, noise_, K, C, t_, s_, _orig=orig, _rec=rec):
        out = _orig(xt, noise_, K, C, t_, s_)
        _rec["t"].append(t_.clone()); _rec["s"].append(s_.clone()); _rec["x"].append(out.clone())
        return out

    dpm.pred_xtms_from_xt = recording
    calls = {"n": 0}
    fwd = m.forward

    def counting(*a, _fwd=fwd, _rec=rec, **k):
        calls["n"] += 1
        out = _fwd(*a, **k)
        _rec["kshare"].append(float((out[0][:, :3].abs() > 1).double().mean()))      # before the sampler's in-place clamp
        return out

    m.forward = counting
    with patched_draws([xT] + epsilons):
        img_ref = dpm.sample_fn((2, 3, 32, 32), unnormalize=True, denoise=denoise)
    m.forward = fwd
    n_steps = 11 if denoise else 10
    assert calls["n"] == n_steps and img_ref.dtype == torch.float32 and rec["t"][0].dtype == torch.float32
    assert float((rec["t"][-1] - rec["s"][-1]).abs().max()) == 0.0
    with torch.no_grad():
        img_o, traj_o, kshare_o = linear_ref.sample_fn(lambda a, b: linear_ref.unet(sd, cfg, a, b), xT, epsilons, 10, EPS, denoise)
    grid = linear_ref.time_grid(10, EPS, denoise)
    tag = f"sample.denoise{int(denoise)}"
    for k in range(n_steps):
        assert float(grid[k][0]) == float(rec["t"][k][0]) and float(grid[k][1]) == float(rec["s"][k][0]), (k, grid[k], rec["t"][k], rec["s"][k])
        check(f"{tag}/state{k}", traj_o[k], rec["x"][k], 1e-4)
    check(tag + "/img", img_o, img_ref, 1e-4)
    g[tag + ".t"] = torch.stack([v[0] for v in rec["t"]]).numpy()
    g[tag + ".s"] = torch.stack([v[0] for v in rec["s"]]).numpy()
    states = torch.stack(rec["x"]).numpy()
    if denoise:
        g[tag + ".states"] = states
    else:       # same x_T, draws and first nine (t, s): the first nine states are those of denoise=True, only the last one is new
        assert np.array_equal(states[:9], g["sample.denoise1.states"][:9])
        g[tag + ".states_from9"] = states[9:]
    g[tag + ".img"] = img_ref.numpy()
    sat = float(((img_ref == 0) | (img_ref == 1)).double().mean())
    report["sampler"][tag] = dict(network_calls=calls["n"], clamped_K_share_per_step=rec["kshare"],
                                  final_pixels_at_0_or_1=sat, restatement_clamped_K_share_per_step=kshare_o)
    print(f"{tag}: clamped K share per step {['%.4f' % v for v in rec['kshare']]}; final pixels at exactly 0 or 1: {sat:.3f}")

np.savez_compressed(os.path.join(OUT, "g17_linear.npz"), **g)
report["all_ok"] = all(c["ok"] for c in report["cases"])
with open(os.path.join(OUT, "oracle_vs_reference_report_linear.json"), "w") as f:
    json.dump(report, f, indent=1)
print("ALL OK", len(report["cases"]), "cases;", os.path.getsize(os.path.join(OUT, "g17_linear.npz")), "bytes")
