"""CPU-only: the LPIPS module's state-dict layout and loaders, its frozen parameters, the wrapper's opt-in rule, and the
conditioning of the fixed inputs that tests/test_hip_lpips.py compares against fp64 (no GPU call is made here)."""
import warnings

import pytest
import torch

import lpips_ref
from oracle import fill

WIDTHS = {"slice1": {0: (64, 3), 2: (64, 64)}, "slice2": {5: (128, 64), 7: (128, 128)},
          "slice3": {10: (256, 128), 12: (256, 256), 14: (256, 256)}, "slice4": {17: (512, 256), 19: (512, 512), 21: (512, 512)},
          "slice5": {24: (512, 512), 26: (512, 512), 28: (512, 512)}}


def expected_layout():
    want = {"scaling_layer.shift": (1, 3, 1, 1), "scaling_layer.scale": (1, 3, 1, 1)}
    for s, convs in WIDTHS.items():
        for i, (co, ci) in convs.items():
            want[f"net.{s}.{i}.weight"] = (co, ci, 3, 3)
            want[f"net.{s}.{i}.bias"] = (co,)
    for k, c in enumerate((64, 128, 256, 512, 512)):
        want[f"lin{k}.model.1.weight"] = (1, c, 1, 1)
    return want


def test_state_dict_layout_is_the_references():
    from adm_amd.ddm.lpips import LPIPS
    m = LPIPS()
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == expected_layout()
    assert len([k for k in got if k.startswith("net.") and k.endswith(".weight")]) == 13
    torch.testing.assert_close(m.scaling_layer.shift.reshape(-1), torch.tensor([-.030, -.088, -.188]))
    torch.testing.assert_close(m.scaling_layer.scale.reshape(-1), torch.tensor([.458, .448, .450]))
    assert {n for n, _ in m.named_buffers()} == {"scaling_layer.shift", "scaling_layer.scale"}
    assert set(lpips_ref.synthetic_state_dict()) == set(got)


def test_no_trainable_parameters_and_stays_in_eval():
    from adm_amd.ddm.lpips import LPIPS
    m = LPIPS()
    assert sum(p.numel() for p in m.parameters()) == 14714688 + 1472      # VGG16 features + the five lin layers
    assert not any(p.requires_grad for p in m.parameters())
    m.train()
    assert not m.training and not any(c.training for c in m.modules())


def test_loaders_round_trip():
    from adm_amd.ddm.lpips import LPIPS
    sd = lpips_ref.synthetic_state_dict()
    a = LPIPS.from_state_dict(sd)
    b = LPIPS.from_state_dict({"perceptual_loss." + k: v for k, v in sd.items()} | {"model.some.weight": torch.zeros(1)})
    vgg = lpips_ref.vgg16_features_state_dict()
    vgg["classifier.0.weight"] = torch.zeros(2, 2)           # a full torchvision state dict has more than `features`
    c = LPIPS.from_vgg16(vgg, lpips_ref.lin_state_dict())
    for m in (a, b, c):
        got = m.state_dict()
        assert set(got) == set(sd)
        for k in sd:
            assert torch.equal(got[k], sd[k]), k
        assert not any(p.requires_grad for p in m.parameters())
    with pytest.raises(RuntimeError):
        LPIPS.from_state_dict({k: v for k, v in sd.items() if k != "net.slice3.12.bias"})


def test_file_loaders(tmp_path):
    from adm_amd.ddm.lpips import LPIPS
    sd = lpips_ref.synthetic_state_dict()
    torch.save({"model": {"perceptual_loss." + k: v for k, v in sd.items()}}, tmp_path / "ckpt.pt")
    torch.save(lpips_ref.vgg16_features_state_dict(), tmp_path / "vgg16.pth")
    torch.save(lpips_ref.lin_state_dict(), tmp_path / "lin.pth")
    for m in (LPIPS.from_file(str(tmp_path / "ckpt.pt")), LPIPS.from_file(str(tmp_path / "vgg16.pth"), str(tmp_path / "lin.pth"))):
        assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())


def test_golden_lin_file_holds_the_five_lin_weights_only():
    sd = lpips_ref.lin_state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {f"lin{k}.model.1.weight": (1, c, 1, 1)
                                                          for k, c in enumerate((64, 128, 256, 512, 512))}
    assert all(float(v.min()) >= 0 for v in sd.values())          # LPIPS lin weights are non-negative by construction


def _small_ddpm(schedule="const", **kw):
    import importlib
    variant = lpips_ref.WRAPPER[schedule][0]
    cfg, sd = lpips_ref.small_unet(schedule)
    keys = ("model_channels", "channel_mult", "channel_mult_emb", "num_blocks", "attn_resolutions", "dropout", "augment_dim")
    unet = importlib.import_module("adm_amd.unet." + variant).EDMPrecond(img_resolution=32, img_channels=3, model_type="DhariwalUNet",
                                                                         **{k: cfg[k] for k in keys})
    D = importlib.import_module("adm_amd.ddm.ddm_" + schedule).DDPM
    return D(model=unet, image_size=[32, 32], sampling_timesteps=2, cfg=dict(eps=1e-4, weighting_loss=True), **kw)


def test_wrapper_without_weights_warns_and_has_no_submodule():
    with pytest.warns(UserWarning, match="loss_vlb is 0"):
        dpm = _small_ddpm(perceptual_weight=1.0)
    assert not hasattr(dpm, "perceptual_loss") and not dpm.lpips_active
    assert not any(k.startswith("perceptual_loss.") for k in dpm.state_dict())
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert not _small_ddpm(perceptual_weight=0.0).lpips_active


def test_wrapper_with_weights_adds_no_trainable_parameter(tmp_path):
    from adm_amd.ddm.lpips import LPIPS
    from adm_amd.optim import FlatParams
    sd = lpips_ref.synthetic_state_dict()
    torch.save(sd, tmp_path / "lpips.pt")
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # no "loss_vlb is 0" warning once weights are supplied
        plain = _small_ddpm(perceptual_weight=0.0)
        by_cfg = _small_ddpm(perceptual_weight=1.0, lpips_ckpt=str(tmp_path / "lpips.pt"))
        by_method = _small_ddpm(perceptual_weight=0.0).set_perceptual_loss(LPIPS.from_state_dict(sd))
    assert by_cfg.lpips_active and not by_method.lpips_active          # perceptual_weight gates the term
    want = [n for n, p in plain.named_parameters() if p.requires_grad]
    for dpm in (by_cfg, by_method):
        assert [n for n, p in dpm.named_parameters() if p.requires_grad] == want
        assert sum(k.startswith("perceptual_loss.") for k in dpm.state_dict()) == 33
        dpm.train()
        assert not dpm.perceptual_loss.training
    assert sum(p.numel() for p in FlatParams(by_cfg).params) == sum(p.numel() for p in FlatParams(plain).params)
    # a checkpoint that carries perceptual_loss.* brings its own VGG16 (and does not when the term is off)
    torch.save({"model": by_cfg.state_dict()}, tmp_path / "model-1.pt")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        from_ckpt = _small_ddpm(perceptual_weight=1.0, ckpt_path=str(tmp_path / "model-1.pt"))
        off = _small_ddpm(perceptual_weight=0.0, ckpt_path=str(tmp_path / "model-1.pt"))
    assert from_ckpt.lpips_active and not hasattr(off, "perceptual_loss")
    assert all(torch.equal(v, sd[k]) for k, v in from_ckpt.perceptual_loss.state_dict().items())


def test_latent_wrapper_has_no_lpips_term():
    from adm_amd.ddm.ddm_const_2 import LatentDiffusion
    assert LatentDiffusion.USES_LPIPS is False


def test_unsupported_sizes_and_modes_raise():
    from adm_amd import ops
    from adm_amd.ddm.lpips import LPIPS
    m = LPIPS()
    with pytest.raises(NotImplementedError, match="multiples of 16"):
        m.features(torch.zeros(1, 24, 32, 32), False)
    old = ops.COMPUTE
    try:
        ops.COMPUTE = "bf16"
        with pytest.raises(NotImplementedError, match="f32"):
            m.features(torch.zeros(1, 32, 32, 32), False)
    finally:
        ops.COMPUTE = old


# ---------------------------------------------------------------------------------------------------------------------------
# conditioning of the GPU tests' fixed inputs: where torch's own fp32 agrees with fp64 this well, a 2e-3 relative-L2 bar on the
# HIP path's gradient leaves a factor of ten above the restatement's own noise (a near-zero pre-activation flips a ReLU or a pool
# choice between two correct fp32 implementations).  An input set that fails gets another seed, never a wider bound.
# ---------------------------------------------------------------------------------------------------------------------------
def _check(rel, grel, zeros, what):
    print(f"{what}: per-sample rel {rel:.2e}, d/dx rel L2 {grel:.2e}, zero-norm positions {zeros}")
    assert rel <= 1e-5 and grel <= 2e-4 and zeros == 0, (what, rel, grel, zeros)


@pytest.mark.parametrize("case", lpips_ref.NETWORK_CASES, ids=lambda c: "B%d_%dx%d_seed%d" % (c[0], c[1], c[1], c[2]))
def test_network_inputs_are_well_conditioned(case):
    x, x0 = lpips_ref.network_inputs(*case)
    _check(*lpips_ref.conditioning(lpips_ref.synthetic_state_dict(), x, x0), f"network inputs {case}")


@pytest.mark.parametrize("schedule", ["const", "const_2"])
def test_wrapper_inputs_are_well_conditioned(schedule):
    """The same condition on the x_rec the oracle's small UNet predicts (the wrapper-level GPU test differentiates through it)."""
    sd = lpips_ref.synthetic_state_dict()
    ref = lpips_ref.oracle_step(schedule, sd)
    assert lpips_ref.GRAD_KEY in ref["grads"] and float(ref["g_vlb"].norm()) > 0
    x0, _, _ = lpips_ref.wrapper_inputs()
    _check(*lpips_ref.conditioning(sd, ref["x_rec"], x0), f"wrapper inputs {schedule}")
