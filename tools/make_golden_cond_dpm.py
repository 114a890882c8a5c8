#!/usr/bin/env python3
"""Golden vectors of the conditional PIXEL-SPACE recipe (train_cond_dpm.py).  RUNS ONLY WHERE THE REFERENCE IS (default
/root/reference, or $ADM_REFERENCE); CPU only.

Imports the reference's own ``ddm.ddm_const_2`` and ``unet.cond_unet`` with the import-time placeholders of
tools/make_golden_linear.py (an 'ADM' package alias) and tools/make_golden_cond2.py (torchvision / fvcore placeholders, a
``pytorch_lightning`` whose ``LightningModule`` is ``torch.nn.Module``), and

  * drives ``ddm.ddm_const_2.DDPM.p_losses`` with use_l1=True, perceptual_weight=0, both weighting_loss settings, a stub model that
    returns recorded predictions, and ``cond`` passed positionally; checks tests/cond_dpm_ref.py (loss, the logged values, both
    prediction gradients) against it;
  * evaluates the 'const' weights (ddm_const.py:336-338; that module itself cannot be imported) on the per-sample terms the SAME
    reference p_losses yields un-weighted -- one sample at a time, with one of the two predictions set to its target, so the call
    returns [SSE_C + mean|e_C|] / 2 or [SSE_eps + mean|e_eps|] / 2 alone -- and checks the restatement's 'const' values;
  * builds the reference's ``unet.cond_unet.Unet`` at channels=1 with injected condition features and checks oracle.cond_unet_ref
    against it: both outputs and every parameter gradient, as g16 does for three channels;
  * measures, on the CPU, how far the fp32 restatement of the one-channel LPIPS network is from fp64 on the inputs of the GPU test
    (tests/lpips_ref.conditioning) and requires the chosen seeds to stay within half of each bar.

Writes tests/golden/g24_cond_dpm.npz (expected outputs only; the inputs are closed-form) and
tests/golden/oracle_vs_reference_report_cond_dpm.json.  The fixtures are data the reference produced; none of its source is copied.
Usage:  python tools/make_golden_cond_dpm.py
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ADM_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)


class _Meta(type):
    def __getattr__(cls, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return cls()


class _Stub(metaclass=_Meta):
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return a[0] if (len(a) == 1 and callable(a[0]) and not k) else self

    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return _Stub()


class _StubModule(types.ModuleType):
    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return _Stub


for name in ["torchvision", "torchvision.ops", "torchvision.ops.misc", "torchvision.ops.stochastic_depth", "torchvision.transforms",
             "torchvision.transforms._presets", "torchvision.utils", "torchvision.models", "torchvision.models._api",
             "torchvision.models._meta", "torchvision.models._utils", "fvcore", "fvcore.common", "fvcore.common.config"]:
    m = _StubModule(name); m.__path__ = []; sys.modules[name] = m


class CfgNode(dict):
    __getattr__ = dict.get


sys.modules["fvcore.common.config"].CfgNode = CfgNode
adm = types.ModuleType("ADM"); adm.__path__ = [REF]; sys.modules["ADM"] = adm
pl = types.ModuleType("pytorch_lightning")
pl.LightningModule = nn.Module                      # base class only
sys.modules["pytorch_lightning"] = pl

import ddm.ddm_const_2 as D2  # noqa: E402  (the reference's pixel-space wrapper)
import unet.cond_unet as C2  # noqa: E402  (the reference's two-decoder denoiser)
import unet.swin_transformer as S  # noqa: E402

S.swin_b = lambda weights=None: None

import cond_dpm_ref as R  # noqa: E402
import lpips_ref  # noqa: E402
from oracle import cond_unet_ref as U  # noqa: E402
from oracle import fill  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.manual_seed(0)
torch.set_num_threads(8)
report = {"torch": torch.__version__, "cases": []}
g = {}


def check(name, got, want, tol=2e-5):
    a, b = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    e = float((a - b).abs().max() / (b.abs().max() + 1e-30))
    ok = e <= tol
    report["cases"].append(dict(case=name, max_rel_err=e, tol=tol, ok=bool(ok)))
    print(f"{'OK ' if ok else 'BAD'} {name}: rel_err={e:.3e}")
    assert ok, name


class patched_draws:
    """torch.randn_like returns the given tensors, in call order."""

    def __init__(self, draws):
        self.it = iter(draws)

    def __enter__(self):
        self.saved = torch.randn_like
        torch.randn_like = lambda *a, **k: next(self.it).clone()

    def __exit__(self, *a):
        torch.randn_like = self.saved


class Recorded(nn.Module):
    """Stands for the denoiser: returns the recorded predictions and keeps what it was called with."""
    channels, self_condition = 1, False

    def __init__(self, c, e):
        super().__init__()
        self.c, self.e, self.seen = c, e, None

    def forward(self, x, t, *args, **kwargs):
        self.seen = (x, t, args, kwargs)
        return self.c, self.e


def ref_p_losses(weighting, x0, t, noise, cond, c, e):
    stub = Recorded(c, e)
    dpm = D2.DDPM(model=stub, image_size=list(x0.shape[-2:]), sampling_timesteps=10, loss_type="l2", start_dist="normal",
                  perceptual_weight=0.0, use_l1=True,
                  cfg=dict(eps=R.EPS, sigma_max=1, sigma_min=0.01, weighting_loss=bool(weighting), use_augment=False))
    dpm.perceptual_weight = 1.0                       # run the reference p_losses un-modified (with 0 its `loss_vlb.sum()` meets a float) ...
    dpm.perceptual_loss = lambda a, b: torch.zeros(a.shape[0], 1, 1, 1)   # ... with LPIPS == 0, as tools/make_golden.py does
    with patched_draws([noise]):
        loss, log = dpm.p_losses(x0, t, cond)
    return loss, log, stub.seen


# ------------------------------------------------------------------------------------------------ p_losses, use_l1, cond, 'const_2'
x0, noise, cond, c, e, t = R.step_inputs()
B = x0.shape[0]
for weighting in R.STEP_VARIANTS:
    cr, er = c.clone().requires_grad_(True), e.clone().requires_grad_(True)
    loss_ref, log_ref, seen = ref_p_losses(weighting, x0, t, noise, cond, cr, er)
    assert len(seen[2]) == 1 and seen[2][0] is cond and not seen[3], "cond must reach the model positionally"
    loss_ref.backward()
    co, eo = c.double().requires_grad_(True), e.double().requires_grad_(True)
    x_noisy = R.q_sample("const_2", x0.double(), noise.double(), t.double())
    loss_o, log_o, simple_o = R.losses("const_2", co, eo, x_noisy, x0.double(), noise.double(), t.double(), R.EPS, bool(weighting))
    loss_o.backward()
    w = torch.stack(R.weights("const_2", t.double(), R.EPS, bool(weighting)), dim=1)
    per_k, dc_k, dn_k = R.ddm_loss_l1(c.double(), e.double(), x0.double(), noise.double(), w, 1.0 / B)
    tag = f"const_2.w{weighting}"
    check(tag + "/x_noisy", x_noisy, seen[0], 1e-6)
    check(tag + "/loss", loss_o, loss_ref)
    for k in log_ref:
        check(tag + "/" + k, log_o[k], log_ref[k])
    check(tag + "/dC_pred", co.grad, cr.grad); check(tag + "/dnoise_pred", eo.grad, er.grad)
    check(tag + "/kernel formula/per-sample", per_k, simple_o.detach(), 1e-12)
    check(tag + "/kernel formula/dC_pred", dc_k, cr.grad); check(tag + "/kernel formula/dnoise_pred", dn_k, er.grad)
    g[tag + ".loss"] = loss_ref.detach().numpy()
    for k in log_ref:
        g[f"{tag}.log.{k}"] = log_ref[k].detach().numpy()
    g[tag + ".dC_pred"], g[tag + ".dnoise_pred"] = cr.grad.numpy().copy(), er.grad.numpy().copy()
g["x_noisy.const_2"] = seen[0].detach().numpy()

# ------------------------------------------------------------------------------------------------ the 'const' weights on the reference's own terms
halves = []          # per sample: ([SSE_C + mean|e_C|] / 2, [SSE_eps + mean|e_eps|] / 2), each from one reference p_losses call
for b in range(B):
    sl = slice(b, b + 1)
    a_c, _, _ = ref_p_losses(0, x0[sl], t[sl], noise[sl], cond[sl], c[sl], noise[sl])
    a_e, _, _ = ref_p_losses(0, x0[sl], t[sl], noise[sl], cond[sl], -x0[sl], e[sl])
    halves.append((a_c.detach().double(), a_e.detach().double()))
for weighting in R.STEP_VARIANTS:
    if weighting:
        t64 = t.double()
        w1 = (t64 ** 2 - t64 + 1) / t64                      # ddm_const.py:336
        w2 = (t64 ** 2 - t64 + 1) / (1 - t64 + R.EPS)        # ddm_const.py:338
    else:
        w1 = w2 = torch.ones(B, dtype=torch.float64)
    want = torch.stack([w1[b] * halves[b][0] + w2[b] * halves[b][1] for b in range(B)])
    wr = R.weights("const", t.double(), R.EPS, bool(weighting))
    got = R.loss_simple(c.double(), e.double(), x0.double(), noise.double(), wr[0], wr[1], True)
    check(f"const.w{weighting}/per-sample loss_simple", got, want)
    g[f"const.w{weighting}.per_sample"] = want.numpy()

# ------------------------------------------------------------------------------------------------ unet.cond_unet.Unet at channels = 1
cfg = U.default_cfg(dim=32, two_decoders=True, channels=1, window_sizes2=[[8, 8], [4, 4], [2, 2], [1, 1]])
m = C2.Unet(dim=cfg["dim"], dim_mults=tuple(cfg["dim_mults"]), cond_dim=cfg["dim"], cond_dim_mults=(), channels=1, cond_in_dim=3,
            window_sizes1=cfg["window_sizes1"], window_sizes2=cfg["window_sizes2"], fourier_scale=cfg["fourier_scale"],
            cfg=CfgNode({"cond_pe": False, "cond_net": "swin"}), cond_net="swin", cond_pe=False)
shapes = U.param_shapes(cfg)
ref = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("init_conv_mask")}
assert ref == {k: tuple(s) for k, s in shapes.items()}, sorted(set(ref) ^ set(shapes))[:10]
assert list(ref) == list(shapes), "registration order differs"
assert ref["init_conv.0.weight"][1] == 129 and ref["final_conv.weight"][0] == 1 and ref["final_conv2.weight"][0] == 1
report["cases"].append(dict(case="unet.c1/state_dict names, shapes and order", max_rel_err=0.0, tol=0.0, ok=True))
sd = U.filled_state_dict(cfg)
missing, unexpected = m.load_state_dict(sd, strict=False)
assert not unexpected and all(k.startswith("init_conv_mask") for k in missing), (missing[:5], unexpected[:5])
for mod in m.modules():
    if isinstance(mod, nn.Dropout):
        mod.p = 0.0
Bu, H = 2, 32
x = fill.hash_tensor((Bu, 1, H, H), "cdpm.unet.x", 1.0)
tt = torch.tensor([0.3, 0.85])
hm = U.cond_features(Bu, H * 4, H * 4, tag="cdpm.hm")          # the photo has the map's size: features at a quarter of each map
m.init_conv_mask = lambda mask: [h.clone() for h in hm]
gx, gy = fill.hash_tensor((Bu, 1, H, H), "cdpm.unet.gx", 1.0), fill.hash_tensor((Bu, 1, H, H), "cdpm.unet.gy", 1.0)
m.eval()
m.zero_grad()
y1, y2 = m(x, tt, None)
assert tuple(y1.shape) == (Bu, 1, H, H) and tuple(y2.shape) == (Bu, 1, H, H)
((y1 * gx).sum() + (y2 * gy).sum()).backward()
sdo = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k and k != "time_mlp.0.W" else v.clone())
       for k, v in sd.items()}
o1, o2 = U.unet_forward(sdo, cfg, x, tt, hm)
((o1 * gx).sum() + (o2 * gy).sum()).backward()
check("unet.c1/x1", o1, y1); check("unet.c1/x2", o2, y2)
g["unet.c1.x1"], g["unet.c1.x2"] = y1.detach().numpy(), y2.detach().numpy()
named = dict(m.named_parameters())
gmax = max(float(p.grad.double().norm()) for k, p in named.items() if p.grad is not None)
worst, n = 0.0, 0
for k, p in named.items():
    if k.startswith("init_conv_mask") or p.grad is None:
        continue
    gn_ref = float(p.grad.double().norm())
    worst, n = max(worst, float((sdo[k].grad.double() - p.grad.double()).norm()) / (gn_ref + 1e-4 * gmax)), n + 1
    g[f"unet.c1.gradnorm.{k}"] = np.array(gn_ref)
report["cases"].append(dict(case=f"unet.c1/all-grad-norms ({n} parameters)", max_rel_err=worst, tol=1e-4, ok=bool(worst < 1e-4)))
print(f"unet.c1: worst gradient rel err over {n} parameters {worst:.2e}")
assert worst < 1e-4
for k in ("init_conv.0.weight", "final_conv.weight", "final_conv2.weight", "final_conv.bias", "ups2.3.3.weight"):
    check(f"unet.c1/grad/{k}", sdo[k].grad, named[k].grad, 1e-4)
    g[f"unet.c1.grad.{k}"] = named[k].grad.reshape(-1)[:4096].numpy().copy()

# ------------------------------------------------------------------------------------------------ one-channel LPIPS: fp32 against fp64 on the CPU
lp_sd = lpips_ref.synthetic_state_dict()
report["lpips_c1_conditioning"] = {}
for B_, size in sorted({(c_[0], c_[1]) for c_ in R.LPIPS_C1_CASES}):
    for seed in range(6):
        xr, xs = R.lpips_c1_inputs(B_, size, seed)
        rel, grel, zeros = lpips_ref.conditioning(lp_sd, xr, xs)
        chosen = (B_, size, seed) in R.LPIPS_C1_CASES
        report["lpips_c1_conditioning"][f"B{B_}_{size}x{size}_seed{seed}"] = dict(value_rel=rel, grad_rel_l2=grel, zero_positions=zeros,
                                                                                  chosen=chosen)
        print(f"lpips c1 B{B_} {size}x{size} seed {seed}: value rel {rel:.2e}, d/dx rel L2 {grel:.2e}, all-zero positions {zeros}"
              + ("  <- chosen" if chosen else ""))
        if chosen:          # half of the bars of tests/test_hip_lpips.py::test_network_vs_fp64 (1e-3, 2e-3)
            ok = rel <= 5e-4 and grel <= 1e-3
            report["cases"].append(dict(case=f"lpips.c1/fp32 restatement within half the bars B{B_} {size} seed {seed}",
                                        max_rel_err=max(rel, grel), tol=1e-3, ok=bool(ok)))
            assert ok, (B_, size, seed, rel, grel)
            per, grad, _ = lpips_ref.value_and_grad(lp_sd, xr, xs, torch.float64)
            g[f"lpips.c1.{size}.per"] = per.numpy()

np.savez_compressed(os.path.join(OUT, "g24_cond_dpm.npz"), **g)
report["all_ok"] = all(c_["ok"] for c_ in report["cases"])
with open(os.path.join(OUT, "oracle_vs_reference_report_cond_dpm.json"), "w") as f:
    json.dump(report, f, indent=1)
print("ALL OK", len(report["cases"]), "cases;", os.path.getsize(os.path.join(OUT, "g24_cond_dpm.npz")), "bytes")
