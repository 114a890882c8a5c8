"""CPU-only checks of the KL autoencoder's training path: the plain-PyTorch restatement (tests/ae_train_ref.py) against the
reference's golden results at fp64, torch fp32's own deviation on the same inputs (the yardstick of the GPU bars), state-dict key
sets with and without enable_training(), the options that must raise, the ``ddm.loss`` alias, and the pure-Python parts of
train_vae.py.  No GPU call is made here.

Restatement vs golden: rtol 1e-9 -- tools/make_golden_ae_train.py measured 0 for every recorded value (tests/golden/
oracle_vs_reference_report_ae_train.json: both sides are fp64 torch on the CPU running the same operations); 1e-9 leaves room
for another torch build's operation order."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import ae_train_ref as R
import lpips_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEPS = {"pre": 0, "post": 3, "clamp": 3, "lvclamp": 3}
CASES = [("pre", 0), ("pre", 1), ("post", 0), ("post", 1), ("clamp", 0), ("lvclamp", 0)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "g18_ae_train.npz"))


def _rel(a, b):
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _l2(a, b):
    a, b = torch.as_tensor(np.asarray(a)).double().reshape(-1), torch.as_tensor(np.asarray(b)).double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def test_report_of_the_golden_generator_is_clean():
    rep = json.load(open(os.path.join(GOLDEN, "oracle_vs_reference_report_ae_train.json")))
    assert len(rep["cases"]) >= 80 and all(c["ok"] and c["max_rel_err"] <= 1e-9 for c in rep["cases"])


@pytest.mark.parametrize("tag,idx", CASES)
def test_restatement_vs_golden_fp64(gold, tag, idx):
    x, eps = R.case_inputs(tag)
    loss, log, grads, sd = R.step_with_grads(R.case_state(tag), lpips_ref.synthetic_state_dict(), R.LOSSCONFIG, x, eps, idx, STEPS[tag])
    key = f"{tag}.opt{idx}"
    assert _rel(loss, gold[f"{key}.loss"]) <= 1e-9
    n = 0
    for k in gold.files:
        if k.startswith(f"{key}.log."):
            assert _rel(log[k[len(key) + 5:]], gold[k]) <= 1e-9, k
            n += 1
        elif k.startswith(f"{key}.grad."):
            assert _rel(grads[k[len(key) + 6:]], gold[k]) <= 1e-9, k
            n += 1
        elif k.startswith(f"{key}.bn."):
            assert _rel(sd["loss.discriminator.main.3." + k[len(key) + 4:]], gold[k]) <= 1e-9, k
    assert n >= (9 if idx == 0 else 4)
    if idx == 0:       # what the cases are for
        ratio = float(gold[f"{key}.log.train/d_weight"]) / R.LOSSCONFIG["disc_weight"]
        assert ratio == 1e4 if tag == "clamp" else 1e-3 < ratio < 1e3
        assert float(gold[f"{key}.log.train/disc_factor"]) == (0.0 if tag == "pre" else 1.0)
    assert int(gold[f"{key}.bn.num_batches_tracked"]) == (1 if idx == 0 else 2)


@pytest.mark.parametrize("tag", ["pre", "post", "lvclamp"])
def test_torch_fp32_deviation_on_the_same_inputs(gold, tag):
    """The yardstick of the GPU bars: how far plain fp32 torch lands from the fp64 golden.  Measured here (torch CPU):
    d_weight 4.2e-7 ('pre'), 1.1e-5 ('post'), 4.3e-6 ('lvclamp') relative, so the GPU bar max(1e-3, 4 x this) is 1e-3; logs
    <= 2.4e-7; worst gradient 6.2e-6 / 2.0e-4 / 5.1e-5 relative L2 (|x - r|, hinge, LeakyReLU, ReLU and max-pool kinks flip single elements), against the GPU bar of 2e-3."""
    x, eps = R.case_inputs(tag)
    _, log, grads, _ = R.step_with_grads(R.case_state(tag), lpips_ref.synthetic_state_dict(), R.LOSSCONFIG, x, eps, 0, STEPS[tag],
                                         dtype=torch.float32)
    key = f"{tag}.opt0"
    dw = _rel(log["train/d_weight"], gold[f"{key}.log.train/d_weight"])
    worst = max(_l2(grads[k[len(key) + 6:]], gold[k]) for k in gold.files if k.startswith(f"{key}.grad."))
    print(f"{tag}: fp32 torch d_weight deviation {dw:.2e}, worst gradient rel L2 {worst:.2e}")
    assert 4 * dw < 1e-3          # so the GPU test's bar max(1e-3, 4 x deviation) is 1e-3
    assert worst < 2e-3 / 4       # the gradient bar leaves room above torch's own fp32 noise
    for k in ("train/total_loss", "train/nll_loss", "train/kl_loss", "train/rec_loss", "train/g_loss"):
        assert _rel(log[k], gold[f"{key}.log.{k}"]) < 1e-3 / 4


# ------------------------------------------------------------------------------------------------ module layout
DD = dict(double_z=True, z_channels=3, resolution=[64, 64], in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2, 4], num_res_blocks=2,
          attn_resolutions=[], dropout=0.0)


def test_state_dict_keys_with_and_without_training():
    from oracle import ae_ref
    ED = importlib.import_module("ddm.encoder_decoder")
    ae = ED.AutoencoderKL(DD, dict(R.LOSSCONFIG), 3)
    plain = list(ae_ref.param_shapes(R.ae_config()).keys())
    assert list(ae.state_dict().keys()) == plain            # exactly today's module: no loss.* entry
    assert ae.loss is None
    ae.enable_training()
    want = plain + ["loss.logvar"] + ["loss.discriminator." + k for k in R.disc_shapes()]
    assert list(ae.state_dict().keys()) == want
    for k, shp in R.disc_shapes().items():
        assert tuple(ae.state_dict()["loss.discriminator." + k].shape) == tuple(shp), k
    # the reference's init: N(0, 0.02) conv weights, N(1, 0.02) BatchNorm weights, zero BatchNorm biases
    w = ae.loss.discriminator.main[8].weight
    assert abs(float(w.std()) - 0.02) < 2e-3 and abs(float(w.mean())) < 1e-3
    bn = ae.loss.discriminator.main[9]
    assert abs(float(bn.weight.mean()) - 1.0) < 5e-3 and float(bn.bias.abs().max()) == 0.0
    # a state dict of the restatement loads strictly, and an installed LPIPS network adds its keys
    sd = R.full_state(R.WSCALE, torch.float32, R.LOGVAR)
    ae.load_state_dict(sd, strict=True)
    from adm_amd.ddm.lpips import LPIPS
    ae.enable_training(lpips=LPIPS.from_state_dict(lpips_ref.synthetic_state_dict()))
    extra = [k for k in ae.state_dict() if k not in want]
    assert extra and all(k.startswith("loss.perceptual_loss.") for k in extra)
    assert "loss.perceptual_loss.lin0.model.1.weight" in extra


def test_checkpoint_with_loss_keys_loads_both_ways(tmp_path):
    ED = importlib.import_module("ddm.encoder_decoder")
    sd = R.full_state(R.WSCALE, torch.float32, R.LOGVAR)
    sd.update({"loss.perceptual_loss." + k: v for k, v in lpips_ref.synthetic_state_dict().items()})
    path = str(tmp_path / "ck.pt")
    torch.save({"model": sd}, path)
    frozen = ED.AutoencoderKL(DD, dict(R.LOSSCONFIG), 3, ckpt_path=path)            # inference: loss.* skipped
    assert frozen.loss is None and not any(k.startswith("loss.") for k in frozen.state_dict())
    ae = ED.AutoencoderKL(DD, dict(R.LOSSCONFIG), 3).enable_training()
    ae.init_from_ckpt(path)
    assert float(ae.loss.logvar) == R.LOGVAR and ae.loss.perceptual_loss is not None
    assert torch.equal(ae.loss.discriminator.main[11].weight, sd["loss.discriminator.main.11.weight"])
    assert torch.equal(ae.state_dict()["loss.perceptual_loss.lin3.model.1.weight"], sd["loss.perceptual_loss.lin3.model.1.weight"])


def test_unsupported_options_raise():
    L = importlib.import_module("ddm.loss")
    ED = importlib.import_module("ddm.encoder_decoder")
    for kw in (dict(disc_loss="vanilla"), dict(use_actnorm=True), dict(disc_conditional=True)):
        with pytest.raises(NotImplementedError):
            L.LPIPSWithDiscriminator(disc_start=1, **kw)
    loss = L.LPIPSWithDiscriminator(disc_start=1)
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(NotImplementedError, match="weights"):
        loss(x, x, None, 0, 0, weights=torch.ones(1))
    with pytest.raises(NotImplementedError, match="cond"):
        loss(x, x, None, 1, 0, cond=x)
    ae = ED.AutoencoderKL(DD, dict(R.LOSSCONFIG), 3)
    with pytest.raises(RuntimeError, match="enable_training"):
        ae.training_step(torch.zeros(1, 3, 64, 64), 0, 0)
    ae.enable_training()
    with pytest.raises(NotImplementedError, match="multiples of 16"):
        ae.training_step(torch.zeros(1, 3, 40, 64), 0, 0)
    from adm_amd import ops
    old = ops.COMPUTE
    try:
        ops.COMPUTE = "bf16"
        with pytest.raises(NotImplementedError, match="bf16"):
            ae.training_step(torch.zeros(1, 3, 64, 64), 0, 0)
    finally:
        ops.COMPUTE = old
    with pytest.raises(NotImplementedError, match="32-bit"):
        ae._check_train_shapes(64, 3, 1024, 1024)
    with pytest.raises(NotImplementedError, match="dropout"):
        ED.AutoencoderKL(dict(DD, dropout=0.1), dict(R.LOSSCONFIG), 3).enable_training()
    with pytest.raises(ValueError):
        ED.AutoencoderKL(DD, None, 3).enable_training()


def test_alias_ddm_loss():
    L = importlib.import_module("ddm.loss")
    from adm_amd.ddm import loss as impl
    assert L.LPIPSWithDiscriminator is impl.LPIPSWithDiscriminator and L.NLayerDiscriminator is impl.NLayerDiscriminator
    from adm_amd.ddm.utils import construct_class_by_name
    m = construct_class_by_name(class_name="ddm.loss.LPIPSWithDiscriminator", disc_start=7, kl_weight=1e-6, disc_weight=0.5)
    assert m.discriminator_iter_start == 7 and m.logvar.shape == () and m.perceptual_loss is None
    assert impl.adopt_weight(1.0, 6, threshold=7) == 0.0 and impl.adopt_weight(1.0, 7, threshold=7) == 1.0


def test_recipe_yaml_matches_the_reference_settings():
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.load(open(os.path.join(root, "configs", "celebahq", "celeb_ae_kl_256x256_d4.yaml")), Loader=yaml.SafeLoader)
    assert cfg["model"]["class_name"] == "ddm.encoder_decoder.AutoencoderKL" and cfg["model"]["embed_dim"] == 3
    assert cfg["model"]["lossconfig"] == dict(disc_start=20001, kl_weight=1e-6, disc_weight=0.5)
    assert cfg["model"]["ddconfig"] == dict(double_z=True, z_channels=3, resolution=[256, 256], in_channels=3, out_ch=3, ch=128,
                                            ch_mult=[1, 2, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)
    t = cfg["trainer"]
    assert (t["gradient_accumulate_every"], t["lr"], t["min_lr"], t["train_num_steps"]) == (2, 5e-6, 1e-6, 50000)
    assert cfg["data"]["class_name"] == "synthetic" and cfg["data"]["batch_size"] == 8


def test_driver_schedule_parts():
    import train_vae as T
    assert T.vae_lr_lambda(0, 5e-6, 1e-6, 50000) == 1.0
    assert T.vae_lr_lambda(25000, 5e-6, 1e-6, 50000) == pytest.approx(0.5 ** 0.95)
    assert T.vae_lr_lambda(49999, 5e-6, 1e-6, 50000) == pytest.approx(0.2)          # the min_lr / lr floor
    assert T.micro_steps(2) == [(0, "opt_ae"), (1, "opt_disc")] and T.micro_steps(1) == [(0, "opt_ae")]
    with pytest.raises(ValueError):
        T.micro_steps(3)
    # EMA.update: every 10th call; copies up to update_after_step; the first update after it copies once more, then averages
    assert T.ema_action(3, False) == (None, False)
    assert T.ema_action(1000, False) == (0.0, False)
    assert T.ema_action(1010, False) == (0.0, True)
    d, init = T.ema_action(1020, True)
    assert init and d == pytest.approx(1 - (1 + 20.0) ** (-2 / 3))
    assert T.ema_action(10 ** 7, True)[0] == 0.995
