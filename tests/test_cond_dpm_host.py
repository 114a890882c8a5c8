"""Host-side checks of the conditional pixel-space recipe (train_cond_dpm.py): no GPU.

1. tests/cond_dpm_ref.py (the fp64 restatement the GPU tests compare against) reproduces tests/golden/g24_cond_dpm.npz, which the
   reference itself produced (tools/make_golden_cond_dpm.py), and oracle.cond_unet_ref at channels = 1 reproduces the reference
   denoiser's outputs stored there.
2. The new C-ABI entries refuse null and misaligned arguments and the linear schedule before any launch.
3. The two YAMLs carry the recipe and construct through the trainer's own pattern; the wrappers accept use_l1; the linear wrapper
   keeps its own use_l1 path.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import yaml

import cond_dpm_ref as R
import lpips_ref
from oracle import cond_unet_ref as U
from oracle import fill
from parity import close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL = -22


@pytest.fixture(scope="module")
def g24():
    return dict(np.load(os.path.join(GOLDEN, "g24_cond_dpm.npz")))


@pytest.fixture(scope="module")
def report():
    with open(os.path.join(GOLDEN, "oracle_vs_reference_report_cond_dpm.json")) as f:
        return json.load(f)


def scalar_close(got, want, what):
    got, want = float(got), float(want)
    assert abs(got - want) <= 1e-5 * abs(want) + 1e-12, (what, got, want)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the restatement against the fixture
# ---------------------------------------------------------------------------------------------------------------------------
def test_report_is_all_ok(report):
    assert report["all_ok"] and all(c["ok"] for c in report["cases"]) and len(report["cases"]) >= 30
    gaps = report["lpips_c1_conditioning"]
    for B, size, seed in R.LPIPS_C1_CASES:          # the measured fp32-against-fp64 gaps of the GPU test's inputs: within half the bars
        e = gaps[f"B{B}_{size}x{size}_seed{seed}"]
        assert e["chosen"] and e["value_rel"] <= 5e-4 and e["grad_rel_l2"] <= 1e-3 and e["zero_positions"] == 0


@pytest.mark.parametrize("weighting", R.STEP_VARIANTS)
def test_restatement_const_2_step(g24, weighting):
    x0, noise, cond, c, e, t = (v.double() for v in R.step_inputs())
    B = x0.shape[0]
    co, eo = c.clone().requires_grad_(True), e.clone().requires_grad_(True)
    seen = []

    def model_fn(x, tt, cd):
        seen.append(cd)
        return co, eo

    loss, log, (x_noisy, _, _) = R.p_losses("const_2", model_fn, x0, t, noise, cond, R.EPS, bool(weighting))
    assert len(seen) == 1 and seen[0] is cond          # the condition reaches the model, positionally
    loss.backward()
    tag = f"const_2.w{weighting}"
    close(x_noisy, g24["x_noisy.const_2"])
    scalar_close(loss.detach(), g24[tag + ".loss"], tag)
    for k in ("train/loss_simple", "train/loss_vlb", "train/loss"):
        scalar_close(log[k], g24[f"{tag}.log.{k}"], (tag, k))
    close(co.grad, g24[tag + ".dC_pred"]); close(eo.grad, g24[tag + ".dnoise_pred"])
    # the kernel's closed form (what adm_ddm_loss_l1 is held to) is the same function
    w = torch.stack(R.weights("const_2", t, R.EPS, bool(weighting)), dim=1)
    per, dc, dn = R.ddm_loss_l1(c, e, x0, noise, w, 1.0 / B)
    scalar_close(per.sum() / B, g24[tag + ".loss"], tag)
    close(dc, g24[tag + ".dC_pred"]); close(dn, g24[tag + ".dnoise_pred"])
    zero = (c + x0) == 0
    assert not bool(zero.any()) or float(dc[zero].abs().max()) == 0.0


@pytest.mark.parametrize("weighting", R.STEP_VARIANTS)
def test_restatement_const_weights(g24, weighting):
    x0, noise, _, c, e, t = (v.double() for v in R.step_inputs())
    w1, w2 = R.weights("const", t, R.EPS, bool(weighting))
    got = R.loss_simple(c, e, x0, noise, w1, w2, True)
    want = torch.from_numpy(g24[f"const.w{weighting}.per_sample"])
    assert float(((got - want).abs() / want.abs()).max()) <= 1e-5


def test_l1_twins_are_means_not_sums():
    c, e, x0, noise, t = (v.double() for v in R.loss_inputs(R.LOSS_SHAPES[0]))
    one = torch.ones_like(t)
    s1, s2, a1, a2 = R.simple_terms(c, e, x0, noise)
    n = x0[0].numel()
    want = (s1 + s2 + ((c + x0).abs().sum([1, 2, 3]) + (e - noise).abs().sum([1, 2, 3])) / n) / 2
    assert torch.allclose(R.loss_simple(c, e, x0, noise, one, one, True), want, rtol=1e-12, atol=0)
    assert int(((c + x0) == 0).sum()) > 0 and int(((e - noise) == 0).sum()) > 0          # the inputs do hold exact zeros


def test_oracle_denoiser_at_one_channel(g24):
    cfg = U.default_cfg(dim=32, two_decoders=True, channels=1, window_sizes2=[[8, 8], [4, 4], [2, 2], [1, 1]])
    sd = U.filled_state_dict(cfg)
    assert sd["init_conv.0.weight"].shape[1] == 129 and sd["final_conv.weight"].shape[0] == 1 and sd["final_conv2.weight"].shape[0] == 1
    x = fill.hash_tensor((2, 1, 32, 32), "cdpm.unet.x", 1.0)
    hm = U.cond_features(2, 128, 128, tag="cdpm.hm")
    with torch.no_grad():
        o1, o2 = U.unet_forward(sd, cfg, x, torch.tensor([0.3, 0.85]), hm)
    close(o1, g24["unet.c1.x1"]); close(o2, g24["unet.c1.x2"])


def test_lpips_restatement_broadcasts_one_channel(g24):
    """taps((x - shift) / scale) with x [B,1,H,W] and shift [1,3,1,1]: three channels from the one, as ScalingLayer does."""
    sd = lpips_ref.synthetic_state_dict()
    B, size, seed = R.LPIPS_C1_CASES[0]
    x, x0 = R.lpips_c1_inputs(B, size, seed)
    per1 = lpips_ref.lpips(lpips_ref.cast(sd, torch.float64), x.double(), x0.double())
    per3 = lpips_ref.lpips(lpips_ref.cast(sd, torch.float64), x.double().expand(-1, 3, -1, -1), x0.double().expand(-1, 3, -1, -1))
    assert torch.equal(per1, per3)
    assert np.allclose(per1.numpy(), g24[f"lpips.c1.{size}.per"], rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the C ABI refuses bad arguments before it launches anything
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from adm_amd import hip
    return hip.lib()


def test_entries_are_declared(lib):
    from adm_amd import hip
    for name in ("adm_ddm_loss_l1", "adm_lpips_input_c1", "adm_lpips_input_c1_bwd"):
        assert name in hip.EXPORTS and hasattr(lib, name)
    assert hip._SIGS["adm_ddm_loss_l1"] == hip._SIGS["adm_ddm_loss"]
    assert hip._SIGS["adm_lpips_input_c1"] == hip._SIGS["adm_lpips_input"]
    assert hip._SIGS["adm_lpips_input_c1_bwd"] == hip._SIGS["adm_lpips_input_bwd"]


def test_ddm_loss_l1_einval(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = [p, p, p, p, p, p, p, p, 0.5, 2, 4, None]
    for i in range(6):          # every required pointer
        a = list(ok); a[i] = None
        assert lib.adm_ddm_loss_l1(*a) == EINVAL, i
    for i in (6, 7):            # one gradient without the other
        a = list(ok); a[i] = None
        assert lib.adm_ddm_loss_l1(*a) == EINVAL, i
    for i, bad in ((9, 0), (9, -1), (10, 0)):
        a = list(ok); a[i] = bad
        assert lib.adm_ddm_loss_l1(*a) == EINVAL, (i, bad)


def test_lpips_input_c1_einval(lib):
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    fwd = [p, p, p, p, p, p, p, 1, 4, 1, None]
    for i in (0, 4, 5, 6):
        a = list(fwd); a[i] = None
        assert lib.adm_lpips_input_c1(*a) == EINVAL, i
    for i in (1, 2, 3):          # schedule 1 needs noise_pred, x_noisy and t
        a = list(fwd); a[i] = None
        assert lib.adm_lpips_input_c1(*a) == EINVAL, i
    a = list(fwd); a[6] = odd
    assert lib.adm_lpips_input_c1(*a) == EINVAL          # y is written with 16-byte stores
    for i, bad in ((7, 0), (8, 0), (9, 2), (9, -2), (9, 3)):          # the linear schedule is not built for one channel
        a = list(fwd); a[i] = bad
        assert lib.adm_lpips_input_c1(*a) == EINVAL, (i, bad)
    bwd = [p, p, p, p, p, 1, 4, 1, None]
    for i in (0, 2, 3):
        a = list(bwd); a[i] = None
        assert lib.adm_lpips_input_c1_bwd(*a) == EINVAL, i
    for i in (1, 4):             # schedule 1 needs t and d_n
        a = list(bwd); a[i] = None
        assert lib.adm_lpips_input_c1_bwd(*a) == EINVAL, i
    a = list(bwd); a[0] = odd
    assert lib.adm_lpips_input_c1_bwd(*a) == EINVAL
    for i, bad in ((5, 0), (6, 0), (7, 2), (7, -2)):
        a = list(bwd); a[i] = bad
        assert lib.adm_lpips_input_c1_bwd(*a) == EINVAL, (i, bad)


def test_ops_lpips_input_refuses_the_linear_schedule_by_name():
    from adm_amd import ops
    sd = lpips_ref.synthetic_state_dict()
    a = torch.zeros(1, 1, 4, 4)
    with pytest.raises(NotImplementedError, match="linear schedule"):
        ops.lpips_input(a, a, a, torch.ones(1), sd["scaling_layer.shift"], sd["scaling_layer.scale"], 2)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. configs and wrappers
# ---------------------------------------------------------------------------------------------------------------------------
def load_yaml(name):
    with open(os.path.join(ROOT, "configs", "saliency", name)) as f:
        return yaml.load(f, Loader=yaml.SafeLoader)


@pytest.mark.parametrize("name,sample", [("duts_cond_ddm_const_dpm.yaml", False), ("duts_cond_ddm_const_dpm_sample.yaml", True)])
def test_committed_yamls_carry_the_recipe(name, sample):
    cfg = load_yaml(name)
    m, u, d, t = cfg["model"], cfg["model"]["unet"], cfg["data"], cfg["trainer"]
    assert m["class_name"] == "ddm.ddm_const.DDPM" and m["image_size"] == [128, 128] and m["sampling_timesteps"] == 10
    assert m["use_l1"] is True and m["weighting_loss"] is True and m["perceptual_weight"] == 1.0 and m["ldm"] is False
    assert "first_stage" not in m and "lpips_ckpt" in m and not m["lpips_ckpt"]
    assert m["eps"] == 1e-4 and m["sigma_min"] == 0.01 and m["start_dist"] == "normal" and m["use_augment"] is False
    assert u["class_name"] == "unet.cond_unet.Unet" and u["dim"] == 128 and u["dim_mults"] == [1, 2, 4, 4] and u["channels"] == 1
    assert u["window_sizes1"] == u["window_sizes2"] == [[8, 8], [4, 4], [2, 2], [1, 1]]
    assert u["fix_bb"] is False and u["cond_encoder"] == "swin_b" and u["train_cond_encoder"] is True and not u["cond_encoder_weights"]
    assert d["class_name"] == "synthetic" and d["synthetic_of"] == "ddm.data.DUTSDataset" and d["image_size"] == [128, 128]
    assert d["batch_size"] == 12 and not d["data_root"]
    assert (t["gradient_accumulate_every"], t["lr"], t["min_lr"], t["train_num_steps"]) == (2, 5e-5, 5e-6, 400000)
    assert t["ema_update_after_step"] == 20000 and t["ema_update_every"] == 4 and t["test_before"] is True
    assert not os.path.isabs(t["results_folder"])
    if sample:
        s = cfg["sampler"]
        assert d["split"] == "test" and d["augment_horizontal_flip"] is False and s["use_ema"] is True
        assert not os.path.isabs(s["ckpt_path"]) and not os.path.isabs(s["save_folder"])
    else:
        assert d["split"] == "train" and d["augment_horizontal_flip"] is True


def test_yaml_class_names_resolve_and_the_recipe_constructs():
    """The pattern of train_uncond_dpm.build_model on the recipe at reduced width, without the encoder (Swin-B is 88M parameters)."""
    import adm_amd.ddm.ddm_const as DC
    import adm_amd.unet.cond_unet as CU
    from adm_amd.ddm.utils import get_obj_by_name
    from train_uncond_dpm import Cfg, build_model
    for name in ("duts_cond_ddm_const_dpm.yaml", "duts_cond_ddm_const_dpm_sample.yaml"):
        cfg = load_yaml(name)
        assert get_obj_by_name(cfg["model"]["class_name"]) is DC.DDPM and get_obj_by_name(cfg["model"]["unet"]["class_name"]) is CU.Unet
        cfg["model"]["unet"].update(dim=32, cond_encoder=None, train_cond_encoder=False)
        with pytest.warns(UserWarning, match="loss_vlb is 0"):
            dpm = build_model(Cfg(cfg).model)
        assert type(dpm) is DC.DDPM and dpm.use_l1 is True and dpm.weighting_loss is True and dpm.channels == 1
        assert dpm.perceptual_weight == 1.0 and not dpm.lpips_active and dpm.SCHEDULE == "const"
        assert tuple(dpm.model.init_conv[0].weight.shape) == (32, 129, 7, 7)
        assert tuple(dpm.model.final_conv.weight.shape) == (1, 32, 1, 1) and tuple(dpm.model.final_conv2.weight.shape) == (1, 32, 1, 1)


def small_unet():
    from adm_amd.unet.uncond_unet import EDMPrecond
    return EDMPrecond(img_resolution=32, img_channels=3, model_channels=64, num_blocks=1, channel_mult=[1, 2, 2, 2], attn_resolutions=[16, 8])


def test_pixel_wrappers_accept_use_l1():
    import adm_amd.ddm.ddm_const as DC
    import adm_amd.ddm.ddm_const_2 as D2
    for D in (DC.DDPM, D2.DDPM):
        dpm = D(model=small_unet(), image_size=[32, 32], perceptual_weight=0.0, use_l1=True, cfg=dict(weighting_loss=True))
        assert dpm.use_l1 is True


def test_linear_wrapper_keeps_its_own_l1_path():
    """ddm.ddm_linear.DDPM has had use_l1 inside adm_ddm_loss_linear all along (tests/test_hip_linear.py); this recipe's kernel is
    not on its path, and what it refused it still refuses."""
    import inspect
    import adm_amd.ddm.ddm_linear as L
    assert "ddm_loss_linear" in inspect.getsource(L.DDPM.p_losses) and "ddm_loss_l1" not in inspect.getsource(L.DDPM.p_losses)
    from adm_amd.unet.uncond_unet import EDMPrecond
    unet = EDMPrecond(img_resolution=32, img_channels=3, model_channels=64, num_blocks=1, channel_mult=[1, 2, 2, 2],
                      attn_resolutions=[16, 8], out_mul=2, precondition=False)
    dpm = L.DDPM(model=unet, image_size=[32, 32], perceptual_weight=0.0, use_l1=True, cfg=dict(weighting_loss=True))
    assert dpm.use_l1 is True
    with pytest.raises(NotImplementedError, match="euler"):
        L.DDPM(model=unet, image_size=[32, 32], perceptual_weight=0.0, use_l1=True, cfg=dict(sample_type="2order"))


def test_train_driver_refuses_what_it_does_not_build(monkeypatch):
    import train_cond_dpm as T
    from adm_amd import ops
    cfg = load_yaml("duts_cond_ddm_const_dpm.yaml")
    T.check_cfg(cfg)
    monkeypatch.setattr(ops, "COMPUTE", "bf16")
    with pytest.raises(NotImplementedError, match="f32 compute mode"):
        T.check_cfg(cfg)
    monkeypatch.setattr(ops, "COMPUTE", "f32")
    ldm = load_yaml("duts_cond_ddm_const_ldm.yaml")
    with pytest.raises(ValueError, match="train_cond_ldm.py"):
        T.check_cfg(ldm)
    cfg["sampler"] = {"test_in_train": True}
    with pytest.raises(NotImplementedError, match="test_in_train"):
        T.check_cfg(cfg)
