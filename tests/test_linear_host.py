"""Host-side checks of the linear-drift DDM (ddm.ddm_linear): no GPU.

1. tests/linear_ref.py (the plain-torch restatement the GPU tests compare against) reproduces every entry of
   tests/golden/g17_linear.npz, which the reference itself produced (tools/make_golden_linear.py).  This pins the restatement to
   the reference where the reference is absent.
2. The recipe configs/cifar10/ddm_uncond_linear_uncond_unet.yaml constructs through the trainer's own pattern.
3. The unsupported combinations raise.
4. Closed forms of the schedule and the sampler's time grid.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

import linear_ref
from parity import close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAML = os.path.join(ROOT, "configs", "cifar10", "ddm_uncond_linear_uncond_unet.yaml")


@pytest.fixture(scope="module")
def g17():
    return dict(np.load(os.path.join(GOLDEN, "g17_linear.npz")))


@pytest.fixture(scope="module")
def report():
    with open(os.path.join(GOLDEN, "oracle_vs_reference_report_linear.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def seen():
    """Fixture keys that test group 1 compared; the last test of the group checks none was left out."""
    return set()


def scalar_close(got, want, what):
    got, want = (float(v.detach()) if isinstance(v, torch.Tensor) else float(v) for v in (got, want))
    assert abs(got - want) <= 1e-3 * abs(want), (what, got, want)


def grad_close(g17, seen, tag, key, grad):
    head, norm = g17[f"{tag}.grad.{key}"], float(g17[f"{tag}.gradnorm.{key}"])
    seen.update({f"{tag}.grad.{key}", f"{tag}.gradnorm.{key}"})
    close(grad.reshape(-1)[:linear_ref.GRAD_HEAD], head, scale=float(grad.abs().max()))
    scalar_close(grad.double().norm(), norm, (tag, key))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the restatement against the fixture
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_aug", [0, 1])
def test_restatement_unet_small(g17, seen, use_aug):
    cfg, sd = linear_ref.small_unet_state()
    x, sigma, aug = linear_ref.unet_inputs()
    sdo = {k: v.clone().requires_grad_(v.is_floating_point() and "resample" not in k) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    theta, noise = linear_ref.unet(sdo, cfg, xo, sigma, **(dict(augment_labels=aug) if use_aug else {}))
    assert tuple(theta.shape) == (2, 6, 32, 32) and tuple(noise.shape) == (2, 3, 32, 32)
    linear_ref.unet_objective(theta, noise).backward()
    tag = f"unet.small.aug{use_aug}"
    close(theta, g17[tag + ".theta_pred"]); close(noise, g17[tag + ".noise_pred"]); close(xo.grad, g17[tag + ".dL_dx"])
    seen.update({tag + ".theta_pred", tag + ".noise_pred", tag + ".dL_dx"})
    for k in linear_ref.GRAD_KEYS:
        if "map_augment" in k and not use_aug:
            continue
        grad_close(g17, seen, tag, k, sdo[k].grad)


def test_restatement_unet_full_width(g17, seen):
    cfg, sd = linear_ref.full_unet_state()
    assert tuple(sd["model.out_conv.weight"].shape) == (6, 192, 3, 3)
    x, sigma, aug = linear_ref.unet_inputs_full()
    with torch.no_grad():
        theta, noise = linear_ref.unet(sd, cfg, x, sigma, augment_labels=aug)
    close(theta, g17["unet.full.theta_pred"]); close(noise, g17["unet.full.noise_pred"])
    seen.update({"unet.full.theta_pred", "unet.full.noise_pred"})


@pytest.mark.parametrize("weighting,use_l1", linear_ref.STEP_VARIANTS)
def test_restatement_training_step(g17, seen, weighting, use_l1):
    cfg, sd = linear_ref.small_unet_state()
    x0, t, noise, K = linear_ref.step_inputs()
    assert 0.25 <= float((K.abs() > 1).double().mean()) <= 0.75
    sdo = {k: v.clone().requires_grad_(v.is_floating_point() and "resample" not in k) for k, v in sd.items()}
    loss, log, x_noisy = linear_ref.p_losses(lambda a, b: linear_ref.unet(sdo, cfg, a, b), x0, t, noise, K, linear_ref.EPS,
                                             bool(weighting), bool(use_l1))
    loss.backward()
    tag = f"step.w{weighting}.l1{use_l1}"
    close(x_noisy, g17["step.x_noisy"]); seen.add("step.x_noisy")
    scalar_close(loss, g17[tag + ".loss"], tag); seen.add(tag + ".loss")
    for k in ("train/loss_simple", "train/loss_vlb", "train/loss"):
        scalar_close(log[k], g17[f"{tag}.log.{k}"], (tag, k)); seen.add(f"{tag}.log.{k}")
    gn = torch.sqrt(sum(v.grad.double().pow(2).sum() for v in sdo.values() if v.grad is not None))
    scalar_close(gn, g17[tag + ".grad_norm"], tag + " gradient norm"); seen.add(tag + ".grad_norm")
    for k in linear_ref.STEP_GRAD_KEYS:
        grad_close(g17, seen, tag, k, sdo[k].grad)


@pytest.mark.parametrize("denoise", [True, False])
def test_restatement_sampler(g17, seen, report, denoise):
    cfg, sd = linear_ref.small_unet_state()
    xT, epsilons = linear_ref.sampler_inputs()
    with torch.no_grad():
        img, traj, kshare = linear_ref.sample_fn(lambda a, b: linear_ref.unet(sd, cfg, a, b), xT, epsilons, linear_ref.SAMPLING_TIMESTEPS,
                                                 linear_ref.EPS, denoise)
    tag = f"sample.denoise{int(denoise)}"
    grid = linear_ref.time_grid(linear_ref.SAMPLING_TIMESTEPS, linear_ref.EPS, denoise)
    assert len(grid) == len(traj) == (11 if denoise else 10)
    # the reference's own float32 cur_time and s per step, bit for bit
    assert np.array_equal(np.array([float(c) for c, _ in grid], dtype=np.float32), g17[tag + ".t"])
    assert np.array_equal(np.array([float(s) for _, s in grid], dtype=np.float32), g17[tag + ".s"])
    states = g17["sample.denoise1.states"] if denoise else np.concatenate([g17["sample.denoise1.states"][:9], g17[tag + ".states_from9"]])
    assert states.shape[0] == len(traj)
    for k, x in enumerate(traj):
        close(x, states[k])
    close(img, g17[tag + ".img"])
    seen.update({tag + ".t", tag + ".s", tag + ".img", "sample.denoise1.states" if denoise else tag + ".states_from9"})
    rep = report["sampler"][tag]
    assert rep["network_calls"] == len(traj)
    # what the report says about the fill (and why the GPU step test draws its own K_pred): few K predictions clamp, half the pixels saturate
    assert max(rep["clamped_K_share_per_step"]) < 0.02 and 0.3 < rep["final_pixels_at_0_or_1"] < 0.7
    sat = float(((img == 0) | (img == 1)).double().mean())
    assert abs(sat - rep["final_pixels_at_0_or_1"]) < 0.01


def test_restatement_covers_every_fixture_entry(g17, seen, report):
    """Runs after the tests above (same module, file order): nothing in the fixture is left uncompared."""
    assert report["all_ok"]
    assert sorted(seen) == sorted(g17), sorted(set(g17) ^ seen)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. construction from the recipe
# ---------------------------------------------------------------------------------------------------------------------------
def build_from_yaml(unet_over=None, model_over=None):
    """The pattern of train_uncond_dpm.py's build_model() on the recipe (as plain dicts), at reduced width."""
    import yaml
    from adm_amd.ddm.utils import construct_class_by_name
    with open(YAML) as f:
        cfg = yaml.load(f, Loader=yaml.SafeLoader)
    model_cfg = cfg["model"]
    model_cfg["unet"].update(dict(model_channels=64, num_blocks=1, **(unet_over or {})))
    model_cfg.update(model_over or {})
    unet = construct_class_by_name(**model_cfg["unet"])
    kw = {k: v for k, v in model_cfg.items() if k not in ("class_name", "unet", "first_stage")}
    return construct_class_by_name(model=unet, cfg=model_cfg, class_name=model_cfg["class_name"], **kw), cfg


def test_recipe_constructs(report):
    import adm_amd.ddm.ddm_linear as L
    with pytest.warns(UserWarning, match="MAE part alone"):
        dpm, cfg = build_from_yaml()
    assert cfg["model"]["class_name"] == "ddm.ddm_linear.DDPM" and cfg["model"]["unet"]["out_mul"] == 2 and cfg["model"]["unet"]["precondition"] is False
    assert type(dpm) is L.DDPM
    assert dpm.image_size == [32, 32] and dpm.channels == 3 and dpm.sampling_timesteps == 10
    assert dpm.weighting_loss is True and dpm.use_l1 is False and dpm.start_dist == "normal" and dpm.perceptual_weight == 1.0
    assert dpm.use_augment and dpm.augment.p == 0.12
    assert not dpm.lpips_active
    assert "eps" in dict(dpm.named_buffers()) and dpm.eps.dtype == torch.float32 and float(dpm.eps) == float(torch.tensor(1e-4))
    assert tuple(dpm.model.model.out_conv.weight.shape) == (6, 64, 3, 3) and tuple(dpm.model.model.out_conv.bias.shape) == (6,)
    assert tuple(dpm.model.model.out_conv2.weight.shape) == (3, 64, 3, 3)
    assert dpm.model.precondition is False
    assert list(dpm.state_dict().keys()) == report["state_dict_keys"]
    twin = copy.deepcopy(dpm)
    assert list(twin.state_dict().keys()) == report["state_dict_keys"]
    assert all(torch.equal(a, b) for a, b in zip(twin.state_dict().values(), dpm.state_dict().values()))


def test_alias_module():
    import ddm.ddm_linear as alias
    import adm_amd.ddm.ddm_linear as L
    assert alias.DDPM is L.DDPM


# ---------------------------------------------------------------------------------------------------------------------------
# 3. what is not supported says so
# ---------------------------------------------------------------------------------------------------------------------------
def test_out_mul_needs_precondition_false():
    from adm_amd.unet.uncond_unet import EDMPrecond
    kw = dict(img_resolution=32, img_channels=3, model_channels=64, num_blocks=1, channel_mult=[1, 2, 2, 2], attn_resolutions=[16, 8])
    with pytest.raises(NotImplementedError, match="precondition: False"):
        EDMPrecond(out_mul=2, **kw)
    with pytest.raises(NotImplementedError, match="precondition: False"):
        EDMPrecond(out_mul=2, precondition=True, **kw)
    m = EDMPrecond(out_mul=2, precondition=False, **kw)
    assert tuple(m.model.out_conv.weight.shape) == (6, 64, 3, 3)


def test_out_mul_rejected_by_single_decoder_variants():
    from adm_amd.unet.uncond_unet_sd import EDMPrecond
    with pytest.raises(NotImplementedError, match="two-decoder"):
        EDMPrecond(img_resolution=32, img_channels=3, model_channels=64, num_blocks=1, channel_mult=[1, 2, 2, 2],
                   attn_resolutions=[16, 8], out_mul=2, precondition=False)


def test_only_the_euler_sampler():
    with pytest.raises(NotImplementedError, match="euler"):
        build_from_yaml(model_over=dict(sample_type="2order", perceptual_weight=0.0))


def test_cond_and_up_scale_raise():
    dpm, _ = build_from_yaml(model_over=dict(perceptual_weight=0.0, use_augment=False))
    with pytest.raises(NotImplementedError):
        dpm.sample(batch_size=1, cond=torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError):
        dpm.sample_fn((1, 3, 32, 32), up_scale=2)
    with pytest.raises(NotImplementedError):
        dpm(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. closed forms
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wrapper():
    dpm, _ = build_from_yaml(model_over=dict(perceptual_weight=0.0, use_augment=False))
    return dpm


def test_q_sample_at_t1_is_the_noise_alone(wrapper):
    """U(1) = K/2 + C = -x0: with zero noise the forward process ends at exactly the origin."""
    g = torch.Generator().manual_seed(3)
    x0 = torch.rand(2, 3, 8, 8, generator=g, dtype=torch.float64) * 2 - 1
    K = torch.randn(2, 3, 8, 8, generator=g, dtype=torch.float64).clamp(-1, 1)
    t = torch.ones(2, dtype=torch.float64)
    C = -x0 - K / 2
    for q in (lambda: wrapper.q_sample(x0, torch.zeros_like(x0), t, K, C), lambda: linear_ref.q_sample(x0, torch.zeros_like(x0), t, K, C)):
        assert float(q().abs().max()) <= 1e-15


def test_pred_x0_inverts_q_sample(wrapper):
    g = torch.Generator().manual_seed(4)
    x0 = torch.rand(3, 3, 8, 8, generator=g, dtype=torch.float64) * 2 - 1
    K = torch.randn(3, 3, 8, 8, generator=g, dtype=torch.float64).clamp(-1, 1)
    noise = torch.randn(3, 3, 8, 8, generator=g, dtype=torch.float64)
    t = torch.tensor([1e-4, 0.4, 0.999], dtype=torch.float64)
    C = -x0 - K / 2
    xt = wrapper.q_sample(x0, noise, t, K, C)
    assert torch.equal(xt, linear_ref.q_sample(x0, noise, t, K, C))
    assert float((wrapper.pred_x0_from_xt(xt, noise, t, K, C) - x0).abs().max()) <= 1e-14
    assert float((linear_ref.x_rec(xt, torch.cat([K, C], 1), noise, t) - x0).abs().max()) <= 1e-14
    # and one reverse step with s = t and no fresh noise lands on x0 + (the part of the drift the step does not remove) = x0 at t -> 0
    z = torch.zeros_like(x0)
    step = wrapper.pred_xtms_from_xt(xt, noise, K, C, t, t, epsilon=z)
    assert torch.allclose(step, linear_ref.sampler_step(xt, torch.cat([K, C], 1), noise, z, t, t), rtol=0, atol=1e-14)


@pytest.mark.parametrize("denoise,n", [(True, 11), (False, 10)])
def test_time_grid(wrapper, denoise, n):
    steps = wrapper.step_grid(denoise)
    assert steps.dtype == torch.float32 and steps.shape[0] == n
    assert abs(float(steps.double().sum()) - 1.0) <= 1e-6
    grid = wrapper.time_grid(denoise)
    assert len(grid) == n and grid[0][0] == 1.0
    ref = linear_ref.time_grid(10, float(wrapper.eps), denoise)
    assert [(float(c), float(s)) for c, s in ref] == grid
    t_last, s_last = grid[-1]
    assert t_last == s_last and t_last > 0                       # the grid ends at exactly zero ...
    assert (s_last * (t_last - s_last) / t_last) ** 0.5 == 0.0     # ... and the last step adds no noise
    if denoise:
        assert abs(t_last - float(wrapper.eps)) <= 1e-6
