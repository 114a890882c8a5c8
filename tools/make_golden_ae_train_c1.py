#!/usr/bin/env python3
"""Golden vectors for the ONE-CHANNEL KL autoencoder's training step: AutoencoderKL(in_channels=1, out_ch=1) with
LPIPSWithDiscriminator(disc_in_channels=1), the first stage of the latent saliency recipe (configs/saliency/DUTS_ae_kl_384x384.yaml
of the reference).  RUNS ONLY WHERE THE REFERENCE CHECKOUT IS AVAILABLE (REF below); same import shims, and the same LPIPS
stand-in, as tools/make_golden_ae_train.py: the reference's own LPIPS() would try to download VGG16 weights and is never
constructed; the name ``LPIPS`` in taming.modules.losses.vqperceptual and ddm.loss is replaced by the fp64 restatement of
tests/lpips_ref.py with its synthetic VGG16 and the real lin weights, whose ScalingLayer broadcasts the one channel to three as
the reference's does ((x - shift[1,3,1,1]) / scale).  Everything else is the reference's code in fp64 on the CPU:
ddm.encoder_decoder.AutoencoderKL and ddm.loss.LPIPSWithDiscriminator with taming's NLayerDiscriminator(input_nc=1).

Cases (tests/ae_train_c1_ref.py: ch = 32, B = 2, 64x48 -- non-square, mid attention L = 192; hash-filled weights; disc_start = 3):
  pre     global_step 0 (< disc_start), both optimizer indices
  post    global_step 3 (>= disc_start), both optimizer indices; the full list of recorded gradients
('pre' records the short list, as g18 does: the four 128x128 attention weights are most of the file).  The d_weight clamp must be
INACTIVE (asserted: 1e-3 < |grad nll| / (|grad g| + 1e-4) < 1e3).

Writes tests/golden/g27_ae_train_c1.npz (no larger than g18_ae_train.npz, asserted) and
tests/golden/oracle_vs_reference_report_ae_train_c1.json (the restatement of tests/ae_train_c1_ref.py against these results).
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

import ae_train_c1_ref as R1  # noqa: E402
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


def build(sd):
    cfg = R1.ae_config()
    assert cfg["in_channels"] == 1 and cfg["out_ch"] == 1 and tuple(cfg["resolution"]) == (64, 48)
    dd = dict(double_z=True, z_channels=cfg["z_channels"], resolution=list(cfg["resolution"]), in_channels=cfg["in_channels"],
              out_ch=cfg["out_ch"], ch=cfg["ch"], ch_mult=list(cfg["ch_mult"]), num_res_blocks=cfg["num_res_blocks"],
              attn_resolutions=[], dropout=0.0)
    ae = ED.AutoencoderKL(dd, dict(R1.LOSSCONFIG), cfg["embed_dim"]).double().train()
    assert isinstance(ae.loss.perceptual_loss, LocalLPIPS)
    assert ae.loss.discriminator.main[0].weight.shape[1] == 1 and ae.decoder.conv_out.weight.shape[0] == 1
    msg = ae.load_state_dict(sd, strict=False)
    assert not msg.unexpected_keys and all(k.startswith("loss.perceptual_loss") for k in msg.missing_keys), msg
    return ae


def ref_step(ae, x, eps, idx, step):
    """AutoencoderKL.training_step (encoder_decoder.py:978-997) with the posterior's draw injected."""
    posterior = ae.encode(x)
    rec = ae.decode(posterior.mean + posterior.std * eps)
    assert rec.shape == x.shape == (R1.BATCH, 1, *R1.RES)
    return ae.loss(x, rec, posterior, idx, step, last_layer=ae.get_last_layer(), split="train")


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def record(name, got, want, tol=1e-9):
    e = rel(got, want)
    report["cases"].append(dict(case=name, max_rel_err=e, tol=tol, ok=bool(e <= tol)))
    print(f"{'OK ' if e <= tol else 'BAD'} {name}: restatement vs reference rel_err={e:.3e}")
    assert e <= tol, name


for tag, idx in R1.CASES:
    step = R1.STEPS[tag]
    x, eps = (t.double() for t in R1.case_inputs(tag))
    ae = build(R1.case_state(tag))
    loss, log = ref_step(ae, x, eps, idx, step)
    ae.zero_grad()
    loss.backward()
    key = f"{tag}.opt{idx}"
    gold[f"{key}.loss"] = loss.detach().numpy()
    for k, v in log.items():
        gold[f"{key}.log.{k}"] = torch.as_tensor(v).detach().double().numpy()
    params = dict(ae.named_parameters())
    names = R1.grad_keys(tag, idx)
    for k in names:
        gold[f"{key}.grad.{k}"] = params[k].grad.detach().numpy()
    after = ae.state_dict()
    for s in ("running_mean", "running_var", "num_batches_tracked"):
        gold[f"{key}.bn.{s}"] = after[f"loss.discriminator.main.3.{s}"].double().numpy()
    if idx == 0:
        ratio = float(log["train/d_weight"]) / R1.LOSSCONFIG["disc_weight"]
        print(f"{key}: |grad nll| / (|grad g| + 1e-4) clamped = {ratio:.4g}, logged d_weight {float(log['train/d_weight']):.6g}")
        assert 1e-3 < ratio < 1e3, f"{key}: the d_weight clamp is active or nearly so ({ratio})"
    # the restatement on the same inputs
    rl, rlog, rgrads, rsd = R1.step_with_grads(R1.case_state(tag), lpips_ref.synthetic_state_dict(), R1.LOSSCONFIG, x, eps, idx, step)
    record(f"{key}.loss", rl, loss.detach())
    for k, v in log.items():
        record(f"{key}.log.{k}", rlog[k], torch.as_tensor(v).detach())
    for k in names:
        record(f"{key}.grad.{k}", rgrads[k], params[k].grad)
    for s in ("running_mean", "running_var", "num_batches_tracked"):
        record(f"{key}.bn.{s}", rsd[f"loss.discriminator.main.3.{s}"], after[f"loss.discriminator.main.3.{s}"])

path = os.path.join(OUT, "g27_ae_train_c1.npz")
np.savez_compressed(path, **gold)
with open(os.path.join(OUT, "oracle_vs_reference_report_ae_train_c1.json"), "w") as f:
    json.dump(report, f, indent=1)
assert os.path.getsize(path) <= os.path.getsize(os.path.join(OUT, "g18_ae_train.npz")), os.path.getsize(path)
print("wrote", len(gold), "arrays,", os.path.getsize(path), "bytes")
