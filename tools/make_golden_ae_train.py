#!/usr/bin/env python3
"""Golden vectors for the KL autoencoder's training step (AutoencoderKL.training_step with LPIPSWithDiscriminator).
RUNS ONLY WHERE THE REFERENCE CHECKOUT IS AVAILABLE (REF below); same import shims as tools/make_golden_latent.py.

The reference's own LPIPS() calls torchvision's vgg16(pretrained=True) and get_ckpt_path(), which try to download: it is NEVER
constructed here.  Before anything is built, the name ``LPIPS`` in taming.modules.losses.vqperceptual and ddm.loss is replaced by
a local module: the fp64 restatement of tests/lpips_ref.py with its synthetic VGG16 and the real lin weights.  Everything else is
the reference's code: ddm.encoder_decoder.AutoencoderKL (Encoder, Decoder, DiagonalGaussianDistribution) and
ddm.loss.LPIPSWithDiscriminator with taming's NLayerDiscriminator, in fp64 on the CPU.  The step is composed as
encoder_decoder.py:978-997 does, with the posterior's draw injected (z = mean + std * eps instead of .sample()'s torch.randn).

Cases (ch = 32, 64x64, B = 2; mid attention C = 128, L = 256; hash-filled weights; disc_start = 3):
  pre     global_step 0 (< disc_start), both optimizer indices
  post    global_step 3 (>= disc_start), both optimizer indices; the full list of recorded gradients
  clamp   global_step 3, optimizer index 0, discriminator weights scaled down until d_weight sits on its 1e4 clamp
  lvclamp global_step 3, optimizer index 0, posterior logvar beyond the [-30, 20] clamp on both sides
In pre / post / lvclamp the d_weight clamp must be INACTIVE (asserted: 1e-3 < |grad nll| / (|grad g| + 1e-4) < 1e3).

Writes tests/golden/g18_ae_train.npz and tests/golden/oracle_vs_reference_report_ae_train.json (the restatement of
tests/ae_train_ref.py against these reference results).
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)
adm = types.ModuleType("ADM"); adm.__path__ = [REF]; sys.modules["ADM"] = adm
tv = types.ModuleType("torchvision"); tv.models = types.ModuleType("torchvision.models")
tv.transforms = types.ModuleType("torchvision.transforms")
sys.modules["torchvision"] = tv; sys.modules["torchvision.models"] = tv.models
sys.modules["torchvision.transforms"] = tv.transforms

import ae_train_ref as R  # noqa: E402
import lpips_ref  # noqa: E402


class LocalLPIPS(torch.nn.Module):
    """Stands in for taming's LPIPS: same call, same [B,1,1,1] result, the restated network with synthetic VGG16 weights."""

    def __init__(self, *a, **k):
        super().__init__()
        self.sd = lpips_ref.cast(lpips_ref.synthetic_state_dict(), torch.float64)

    def forward(self, input, target):
        return lpips_ref.lpips(self.sd, input, target).reshape(-1, 1, 1, 1)


import taming.modules.losses.vqperceptual as VQP  # noqa: E402
VQP.LPIPS = LocalLPIPS
import ddm.loss as RL  # noqa: E402
RL.LPIPS = LocalLPIPS
import ddm.encoder_decoder as ED  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)
report = {"torch": torch.__version__, "cases": []}
gold = {}

CASES = {"pre": dict(step=0, idx=(0, 1), full=False),
         "post": dict(step=3, idx=(0, 1), full=True),
         "clamp": dict(step=3, idx=(0,), full=False, clamp=True),
         "lvclamp": dict(step=3, idx=(0,), full=False, lvclamp=True)}


def build(sd):
    cfg = R.ae_config()
    dd = dict(double_z=True, z_channels=cfg["z_channels"], resolution=list(cfg["resolution"]), in_channels=cfg["in_channels"],
              out_ch=cfg["out_ch"], ch=cfg["ch"], ch_mult=list(cfg["ch_mult"]), num_res_blocks=cfg["num_res_blocks"],
              attn_resolutions=[], dropout=0.0)
    ae = ED.AutoencoderKL(dd, dict(R.LOSSCONFIG), cfg["embed_dim"]).double().train()
    assert isinstance(ae.loss.perceptual_loss, LocalLPIPS)
    msg = ae.load_state_dict(sd, strict=False)
    assert not msg.unexpected_keys and all(k.startswith("loss.perceptual_loss") for k in msg.missing_keys), msg
    return ae


def ref_step(ae, x, eps, idx, step):
    """AutoencoderKL.training_step (encoder_decoder.py:978-997) with the posterior's draw injected."""
    posterior = ae.encode(x)
    rec = ae.decode(posterior.mean + posterior.std * eps)
    return ae.loss(x, rec, posterior, idx, step, last_layer=ae.get_last_layer(), split="train")


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def record(name, got, want, tol=1e-9):
    e = rel(got, want)
    report["cases"].append(dict(case=name, max_rel_err=e, tol=tol, ok=bool(e <= tol)))
    print(f"{'OK ' if e <= tol else 'BAD'} {name}: restatement vs reference rel_err={e:.3e}")
    assert e <= tol, name


for tag, c in CASES.items():
    x, eps = (t.double() for t in R.case_inputs(tag))
    for idx in c["idx"]:
        sd = R.case_state(tag)
        ae = build(sd)
        loss, log = ref_step(ae, x, eps, idx, c["step"])
        ae.zero_grad()
        loss.backward()
        key = f"{tag}.opt{idx}"
        gold[f"{key}.loss"] = loss.detach().numpy()
        for k, v in log.items():
            gold[f"{key}.log.{k}"] = torch.as_tensor(v).detach().double().numpy()
        params = dict(ae.named_parameters())
        names = (R.GRAD_KEYS if c["full"] else R.GRAD_KEYS_SMALL) if idx == 0 else (R.DISC_GRAD_KEYS if c["full"] else R.DISC_GRAD_KEYS[:1])
        for k in names:
            gold[f"{key}.grad.{k}"] = params[k].grad.detach().numpy()
        # the parameters the OTHER optimizer owns: the reference's backward reaches them too (nothing is detached at optimizer
        # index 0), which is why its driver zeroes gradients per optimizer; not recorded
        after = ae.state_dict()
        for s in ("running_mean", "running_var", "num_batches_tracked"):
            gold[f"{key}.bn.{s}"] = after[f"loss.discriminator.main.3.{s}"].double().numpy()
        if idx == 0:
            ratio = float(log["train/d_weight"]) / R.LOSSCONFIG["disc_weight"]
            print(f"{key}: |grad nll| / (|grad g| + 1e-4) clamped = {ratio:.4g}, logged d_weight {float(log['train/d_weight']):.6g}")
            if c.get("clamp"):
                assert ratio == 1e4, ratio
            else:
                assert 1e-3 < ratio < 1e3, f"{key}: the d_weight clamp is active or nearly so ({ratio})"
            if c.get("lvclamp"):
                lv = torch.chunk(ae.quant_conv(ae.encoder(x)), 2, dim=1)[1]
                assert (lv > 20).any() and (lv < -30).any()
        # the restatement on the same inputs
        rl, rlog, rgrads, rsd = R.step_with_grads(R.case_state(tag), lpips_ref.synthetic_state_dict(), R.LOSSCONFIG, x, eps, idx, c["step"])
        record(f"{key}.loss", rl, loss.detach())
        for k, v in log.items():
            record(f"{key}.log.{k}", rlog[k], torch.as_tensor(v).detach())
        for k in names:
            record(f"{key}.grad.{k}", rgrads[k], params[k].grad)
        for s in ("running_mean", "running_var", "num_batches_tracked"):
            record(f"{key}.bn.{s}", rsd[f"loss.discriminator.main.3.{s}"], after[f"loss.discriminator.main.3.{s}"])

np.savez_compressed(os.path.join(OUT, "g18_ae_train.npz"), **gold)
with open(os.path.join(OUT, "oracle_vs_reference_report_ae_train.json"), "w") as f:
    json.dump(report, f, indent=1)
print("wrote", len(gold), "arrays,", os.path.getsize(os.path.join(OUT, "g18_ae_train.npz")), "bytes")
