"""GPU: the Swin condition encoder on HIP kernels against the float64 outputs of the reference's own classes
(tests/golden/g19_swin.npz): the fused window attention, LayerNorm with weight and bias, PatchMerging's gather + LayerNorm, the
small model and Swin-B end to end, run-to-run bit equality, a 2-step conditional latent sample through
``Unet(cond_encoder="swin_b")`` and the sample_cond_ldm.py CLI with ``sampler.cond_encoder: swin_b``.  Every comparison is at the
project's bar (tests/parity.close: rtol 1e-3 / atol 1e-4)."""
import importlib
import os
import subprocess
import sys

import pytest
import torch
import yaml

import swin_ref as R
from oracle import ae_ref, fill
from oracle import cond_unet_ref as CR
from parity import close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _f32(t, gpu):
    return t.to(torch.float32).to(gpu).contiguous()


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_window_attention_vs_reference(gpu, golden, name):
    from adm_amd import ops_swin as osw
    qkv, qb, table, heads, shift = R.attn_case_core(name)
    out = osw.window_attention(_f32(qkv, gpu), _f32(qb, gpu), _f32(table, gpu), heads, shift)
    B, H, W, C, _, _ = R.ATTN_CASES[name]
    assert tuple(out.shape) == (B, H, W, C)
    close(R.sample(out.cpu()), golden[f"attn.{name}"])


def test_window_attention_refuses_other_windows_and_head_widths(gpu):
    from adm_amd import ops_swin as osw
    z = lambda *s: torch.zeros(*s, device=gpu)
    with pytest.raises(RuntimeError):
        osw.window_attention(z(1, 8, 8, 96), z(96), z(225, 1), 1, 0, window=8)
    with pytest.raises(RuntimeError):
        osw.window_attention(z(1, 7, 7, 192), z(192), z(169, 1), 1, 0)          # one head of 64 channels
    with pytest.raises(RuntimeError):
        osw.window_attention(z(1, 7, 7, 96), z(96), z(169, 1), 1, 7)            # shift >= window


@pytest.mark.parametrize("C", [32, 128, 512, 1024, 2048])
def test_layer_norm_affine(gpu, C):
    """37 rows (more than one workgroup, a partial last one): plain rows, rows on a common offset of 300 (the mean is then 500
    times the spread), rows that are zero except for a few entries, and a constant row."""
    from adm_amd import ops_swin as osw
    M = 37
    x = fill.hash_tensor((M, C), f"ln.x{C}", 1.0, torch.float64)
    x[5:12] += 300.0
    x[12:15] -= 1000.0
    x[15:20] = 0.0
    x[15:20, 3] = 2.5
    x[17, C - 1] = -40.0
    x[20] = 7.0
    x = x.to(torch.float32)
    w = 1.0 + fill.hash_tensor((C,), f"ln.w{C}", 0.1, torch.float64)
    b = fill.hash_tensor((C,), f"ln.b{C}", 0.1, torch.float64)
    want = R.layer_norm(x.double(), w, b)
    got = osw.layer_norm(x.to(gpu), _f32(w, gpu), _f32(b, gpu))
    close(got, want)
    close(got[20], b)                     # a constant row: exactly the bias


@pytest.mark.parametrize("name", list(R.MERGE_CASES))
def test_patch_merging_vs_reference(gpu, golden, name):
    from adm_amd import ops, ops_swin as osw
    x, sd = R.merge_case_inputs(name)
    B, H, W, C = R.MERGE_CASES[name]
    ln = osw.merge_layer_norm(_f32(x, gpu), _f32(sd[name + ".norm.weight"], gpu), _f32(sd[name + ".norm.bias"], gpu))
    assert tuple(ln.shape) == (B, (H + 1) // 2, (W + 1) // 2, 4 * C)
    close(R.sample(ln.cpu()), golden[f"merge.{name}.ln"])
    out = ops.linear(ln.reshape(-1, 4 * C), _f32(sd[name + ".reduction.weight"], gpu), None)
    close(R.sample(out.cpu()), golden[f"merge.{name}.out"])


def _model(cfg, gpu):
    from adm_amd.unet.swin_transformer import SwinTransformer
    m = SwinTransformer(patch_size=[4, 4], embed_dim=cfg["embed_dim"], depths=list(cfg["depths"]), num_heads=list(cfg["num_heads"]),
                        window_size=[7, 7])
    m.load_state_dict(R.filled_state_dict(**cfg, dtype=torch.float32), strict=True)
    return m.to(gpu)


@pytest.fixture(scope="module")
def small(gpu):
    return _model(R.SMALL, gpu)


@pytest.fixture(scope="module")
def swin_b_filled(gpu):
    return _model(R.SWIN_B, gpu)


def _check_model(m, name, shape, golden, gpu):
    ys = m(R.model_input(name, shape, torch.float32).to(gpu))
    assert [list(y.shape) for y in ys] == golden[f"{name}.shapes"].tolist()
    for i, y in enumerate(ys):
        assert y.dtype == torch.float32 and y.is_contiguous()
        close(R.sample(y.cpu()), golden[f"{name}.stage{i}"])
    return ys


def test_small_model_end_to_end(small, golden, gpu):
    m = small.train()                     # eval semantics whatever the mode
    _check_model(m, "small", R.SMALL_INPUT, golden, gpu)
    m.eval()


def test_small_model_is_bit_reproducible(small, gpu):
    x = R.model_input("small", R.SMALL_INPUT, torch.float32).to(gpu)
    a, b = small(x), small(x)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("name", list(R.SWIN_B_INPUTS))
def test_swin_b_end_to_end(swin_b_filled, golden, gpu, name):
    _check_model(swin_b_filled, name, R.SWIN_B_INPUTS[name], golden, gpu)


def test_two_step_sample_through_the_builtin_encoder(gpu):
    """ldm.sample with the condition IMAGE (the denoiser runs its init_conv_mask in every step) == the same call given the
    encoder's four feature maps as a precomputed list; 32x32 latents, 128x128 output, two decoders."""
    ED = importlib.import_module("ddm.encoder_decoder")
    D = importlib.import_module("ddm.ddm_const")
    U = importlib.import_module("unet.cond_unet")
    from adm_amd.unet.swin_transformer import SwinTransformer
    dd = dict(double_z=True, z_channels=3, resolution=[128, 128], in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2, 4], num_res_blocks=2,
              attn_resolutions=[], dropout=0.0)
    ae = ED.AutoencoderKL(dd, dict(disc_start=50001, kl_weight=1e-6, disc_weight=0.5), 3)
    ae.load_state_dict(fill.filled_state_dict(ae_ref.param_shapes(ae_ref.ae_cfg(ch=32, resolution=(128, 128)))), strict=True)
    cfg = CR.default_cfg(dim=32, two_decoders=True)
    unet = U.Unet(dim=32, dim_mults=cfg["dim_mults"], cond_dim=32, cond_dim_mults=(), channels=3, cond_in_dim=3,
                  window_sizes1=cfg["window_sizes1"], window_sizes2=cfg["window_sizes2"], fourier_scale=16, cfg={"cond_net": "swin"},
                  cond_encoder="swin_b", fix_bb=True)
    assert isinstance(unet.init_conv_mask, SwinTransformer)
    msg = unet.load_state_dict(CR.filled_state_dict(cfg), strict=False)
    assert not msg.unexpected_keys and all(k.startswith("init_conv_mask.") for k in msg.missing_keys)
    mcfg = dict(eps=1e-4, sigma_max=1, sigma_min=0.01, weighting_loss=True, use_augment=False, ldm=True)
    ldm = D.LatentDiffusion(auto_encoder=ae, scale_factor=0.195, scale_by_std=True, default_scale=True, model=unet,
                            image_size=[128, 128], sampling_timesteps=2, loss_type="l2", start_dist="normal",
                            perceptual_weight=0.0, use_l1=True, cfg=dict(mcfg)).to(gpu).eval()
    B = 2
    cond = fill.hash_tensor((B, 3, 32, 32), "swin.cond", 1.0).to(gpu)
    xT = fill.hash_tensor((B, 3, 32, 32), "swin.xT", 1.7, torch.float64).to(gpu)
    feats = unet.init_conv_mask(cond)
    assert [tuple(f.shape) for f in feats] == [(B, 128, 8, 8), (B, 256, 4, 4), (B, 512, 2, 2), (B, 1024, 1, 1)]
    assert float(feats[0].abs().max()) > 0
    a = ldm.sample(cond=cond, x_T=xT)
    b = ldm.sample(cond=[f.clone() for f in feats], x_T=xT)
    assert a.shape == (B, 3, 128, 128) and bool(torch.isfinite(a).all())
    assert torch.equal(a, b)


def test_sample_cond_ldm_cli_with_the_builtin_encoder(tmp_path):
    """sampler.cond_encoder: swin_b from a checkpoint written here that holds init_conv_mask.* -> PNGs; the same checkpoint
    without those tensors is refused."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from train_uncond_dpm import Cfg, build_model
    from adm_amd.unet.swin_transformer import swin_b
    cfg = yaml.load(open(os.path.join(ROOT, "configs/super-resolution/div2k_cond_ddm_const_ldm.yaml")), Loader=yaml.SafeLoader)
    cfg["model"].update(image_size=[64, 64], sampling_timesteps=2)
    cfg["model"]["first_stage"]["ddconfig"].update(ch=32, resolution=[64, 64])
    cfg["model"]["unet"].update(dim=32, class_name="unet.cond_unet_sd.Unet", window_sizes1=[[2, 2], [1, 1], [1, 1], [1, 1]],
                                window_sizes2=[[4, 4], [2, 2], [1, 1], [1, 1]])
    cfg["data"].update(image_size=[62, 78])
    out = str(tmp_path / "png")
    ckpt, bare = str(tmp_path / "with_encoder.pt"), str(tmp_path / "without_encoder.pt")
    cfg["sampler"].update(sample_num=1, crop_size=[16, 16], stride=[8, 8], save_folder=out, cond_encoder="swin_b", window_batch=0,
                          ckpt_path=ckpt, use_ema=False)
    ldm = build_model(Cfg(cfg).model)
    sd = {k: v for k, v in ldm.state_dict().items()}
    assert not any(".init_conv_mask." in k for k in sd)
    torch.save({"model": sd}, bare)
    enc = swin_b()
    with torch.no_grad():
        enc.first_coonv[0].bias.fill_(0.25)          # (the default initialisation zeroes every bias)
    sd.update({"model.init_conv_mask." + k: v for k, v in enc.state_dict().items()})
    torch.save({"model": sd}, ckpt)
    path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sample_cond_ldm.py"), "--cfg", path], capture_output=True, text=True, env=env,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "PSNR:" in r.stdout and "0 missing, 0 unexpected" in r.stdout, r.stdout[-2000:]
    from PIL import Image
    names = sorted(os.listdir(out))
    assert names == [f"{0: 010d}.png"], names
    assert Image.open(os.path.join(out, names[0])).size == (78, 62)
    cfg["sampler"].update(ckpt_path=bare)
    yaml.safe_dump(cfg, open(path, "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sample_cond_ldm.py"), "--cfg", path], capture_output=True, text=True, env=env,
                       timeout=900)
    assert r.returncode != 0 and "lacks" in (r.stdout + r.stderr) and "init_conv_mask" in (r.stdout + r.stderr)
