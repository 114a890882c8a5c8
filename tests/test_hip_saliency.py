"""GPU: the saliency recipe (configs/saliency/duts_cond_ddm_const_ldm.yaml) above its batch source -- the ONE-channel KL first stage
against oracle.ae_ref, unet.cond_unet.Unet at the recipe's shape family (maps that are multiples of 3, not powers of two) against
oracle.cond_unet_ref, one training step on a DUTSBatchStream batch against the hand-assembled batch, and train_cond_ldm.py /
sample_cond_ldm.py end to end on a small DUTS tree.  Reduced recipe: 192x192 images, a ch = 32 first stage (48x48 latents), dim 32,
Swin-B built in."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import duts_data_ref as R
from oracle import ae_ref, fill
from oracle import cond_unet_ref as C
from parity import close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def test_one_channel_first_stage_vs_oracle(gpu):
    """AutoencoderKL at in_channels 1 / out_ch 1 (no config built it before): the posterior's mode and the decoder against the CPU
    oracle on hash-filled weights, at the bars tests/test_hip_latent.py holds the three-channel one to."""
    ED = importlib.import_module("ddm.encoder_decoder")
    res = (64, 64)
    cfg = ae_ref.ae_cfg(ch=32, resolution=res, in_channels=1, out_ch=1)
    dd = dict(double_z=True, z_channels=3, resolution=list(res), in_channels=1, out_ch=1, ch=32, ch_mult=[1, 2, 4], num_res_blocks=2,
              attn_resolutions=[], dropout=0.0)
    ae = ED.AutoencoderKL(dd, dict(disc_start=50001, kl_weight=1e-6, disc_weight=0.5, disc_in_channels=1), 3)
    sd = fill.filled_state_dict(ae_ref.param_shapes(cfg))
    assert sd["encoder.conv_in.weight"].shape[1] == 1 and sd["decoder.conv_out.weight"].shape[0] == 1
    ae.load_state_dict(sd, strict=True)
    ae = ae.to(gpu).eval()
    x = fill.hash_tensor((2, 1, *res), "sal.ae.x", 1.0)
    z = fill.hash_tensor((2, 3, 16, 16), "sal.ae.z", 1.0)
    with torch.no_grad():
        moments = ae_ref.encode_moments(sd, cfg, x)
        rec = ae_ref.decode(sd, cfg, z)
    assert tuple(moments.shape) == (2, 6, 16, 16) and tuple(rec.shape) == (2, 1, *res)
    post = ae.encode(x.to(gpu))
    close(post.parameters, moments)
    close(post.mode(), moments[:, :3], scale=float(moments.abs().max()))
    got = ae.decode(z.to(gpu))
    assert tuple(got.shape) == (2, 1, *res)
    close(got, rec)


def test_denoiser_at_the_recipe_shape_family_vs_oracle(gpu):
    """unet.cond_unet.Unet with dim 32 x (1, 2, 4, 4), windows 8 / 4 / 2 / 1 on both sides, a 48x48 latent (maps 48 / 24 / 12: the
    recipe's 96 / 48 / 24 halved), B = 1, the four condition maps given directly: forward, the gradients of every input, and the
    gradients of the weights against the CPU oracle, as tests/test_hip_cond.py holds the two-decoder model at 32x32."""
    wins = [[8, 8], [4, 4], [2, 2], [1, 1]]
    cfg = C.default_cfg(dim=32, two_decoders=True, window_sizes1=wins, window_sizes2=wins)
    mod = importlib.import_module("unet.cond_unet")
    m = mod.Unet(dim=32, dim_mults=cfg["dim_mults"], cond_dim=32, cond_dim_mults=(), channels=3, cond_in_dim=3, window_sizes1=wins,
                 window_sizes2=wins, fourier_scale=16, cfg={"cond_net": "swin", "cond_pe": False})
    sd = C.filled_state_dict(cfg)
    m.load_state_dict(sd, strict=True)
    for mm in m.modules():
        if isinstance(mm, torch.nn.Dropout):
            mm.p = 0.0
    m = m.to(gpu).eval()
    x = fill.hash_tensor((1, 3, 48, 48), "sal.x", 1.0)
    tt = torch.tensor([0.4])
    hm = C.cond_features(1, 192, 192, tag="sal.hm")
    assert [tuple(h.shape[2:]) for h in hm] == [(48, 48), (24, 24), (12, 12), (6, 6)]
    gx, gy = fill.hash_tensor((1, 3, 48, 48), "sal.gx", 1.0), fill.hash_tensor((1, 3, 48, 48), "sal.gy", 1.0)
    xg = x.to(gpu).requires_grad_(True)
    hg = [h.to(gpu).requires_grad_(True) for h in hm]
    y1, y2 = m(xg, tt.to(gpu), hg)
    sdo = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k and k != "time_mlp.0.W" else v.clone())
           for k, v in sd.items()}
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
    for name in (names[0], names[len(names) // 4], names[len(names) // 2], names[3 * len(names) // 4], names[-1]):
        want = sdo[name].grad
        close(named[name].grad, want, scale=max(float(want.double().norm()) / 8, 1e-12))


SIZES = [((150, 230), (150, 230)), ((260, 171), (240, 180)), ((192, 192), (192, 192)), ((201, 333), (201, 333)),
         ((300, 250), (300, 250)), ((170, 192), (170, 192))]


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
            Image.fromarray(R.hash_bytes((ph, pw, 3), f"sal.tree.p{i}")).save(img_dir / f"img_{i}.jpg", quality=90)
            Image.fromarray(R.hash_bytes((mh, mw), f"sal.tree.m{i}")).save(mask_dir / f"img_{i}.png")
            back[split_dir].append((np.asarray(Image.open(img_dir / f"img_{i}.jpg").convert("RGB")),
                                    np.asarray(Image.open(mask_dir / f"img_{i}.png").convert("L"))))
    return back


def reduced_cfg(tmp_path):
    cfg = yaml.load(open(os.path.join(ROOT, "configs/saliency/duts_cond_ddm_const_ldm_sample.yaml")), Loader=yaml.SafeLoader)
    u = cfg["model"]["unet"]
    assert u["cond_encoder"] == "swin_b" and u["train_cond_encoder"] is True and u["dim"] == 128 and u["dim_mults"] == [1, 2, 4, 4]
    assert cfg["model"]["first_stage"]["ddconfig"]["in_channels"] == 1 and cfg["model"]["first_stage"]["ddconfig"]["out_ch"] == 1
    cfg["model"].update(image_size=[192, 192], sampling_timesteps=2)
    cfg["model"]["first_stage"]["ddconfig"].update(ch=32, resolution=[192, 192])
    u.update(dim=32, cond_feature_size=[48, 48])
    cfg["data"].update(class_name="ddm.data.DUTSDataset", data_root=str(tmp_path / "duts"), split="train", image_size=[192, 192],
                       batch_size=2, augment_horizontal_flip=True)
    res = str(tmp_path / "run")
    cfg["trainer"].update(results_folder=res, gradient_accumulate_every=2, train_num_steps=3, save_and_sample_every=2, log_freq=1,
                          test_before=True, ema_update_after_step=1, ema_update_every=1, resume_milestone=0)
    cfg["sampler"].update(sample_num=2, cond_encoder="swin_b", use_ema=True, ckpt_path=os.path.join(res, "model-1.pt"),
                          save_folder=os.path.join(res, "png"))
    del cfg["sampler"]["crop_size"], cfg["sampler"]["stride"]          # as the reference's YAML: the defaults are one window, the image
    return cfg, res


def test_training_step_sees_the_reference_batch(gpu, tmp_path):
    """One step in process: the batch DUTSBatchStream makes of injected draws is torch.equal to the batch assembled by hand from
    tests/duts_data_ref.py, and both give the model the same finite positive loss (tests/parity.close)."""
    from adm_amd.ddm.pair_data import DUTSBatchStream
    from train_uncond_dpm import Cfg, build_model
    back = duts_tree(tmp_path / "duts")["DUTS-TR"]
    cfg, _ = reduced_cfg(tmp_path)
    cfg = Cfg(cfg)
    torch.manual_seed(21)
    ldm = build_model(cfg.model).to(gpu).eval()          # (eval: the denoiser's dropout seeds advance from call to call)
    ldm.model.init_conv_mask.train()                     # stochastic depth stays on: its draws come from the seeded device generator
    stream = DUTSBatchStream(cfg.data, 2, (192, 192), gpu, seed=5)
    idx, flip = [1, 3], [1, 0]
    batch = stream.next_batch(idx=idx, flip=flip)
    pairs = [R.duts_pair(*back[i], (192, 192), flip=bool(f)) for i, f in zip(idx, flip)]
    hand = {"image": R.gray_to_float(np.stack([p[1] for p in pairs])).to(gpu), "cond": R.to_float(np.stack([p[0] for p in pairs])).to(gpu)}
    assert list(batch) == ["image", "cond"]
    assert tuple(batch["image"].shape) == (2, 1, 192, 192) and tuple(batch["cond"].shape) == (2, 3, 192, 192)
    assert torch.equal(batch["image"], hand["image"]) and torch.equal(batch["cond"], hand["cond"])
    ldm.on_train_batch_start(batch)
    t = torch.tensor([0.3, 0.7], device=gpu)
    noise, eps = (fill.hash_tensor((2, 3, 48, 48), f"sal.train.{k}", 1.0).to(gpu) for k in ("noise", "eps"))
    losses = []
    for b in (batch, hand):
        torch.manual_seed(22)
        loss, log = ldm.training_step(b, eps=eps, t=t, noise=noise)
        losses.append(loss.detach())
    print(f"losses {float(losses[0]):.6f} / {float(losses[1]):.6f}")
    assert bool(torch.isfinite(losses[0])) and float(losses[0]) > 0
    close(losses[0], losses[1])


def test_train_and_sample_saliency_cli_end_to_end(gpu, tmp_path):
    from PIL import Image
    duts_tree(tmp_path / "duts")
    cfg, res = reduced_cfg(tmp_path)
    path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "train_cond_ldm.py"), "--cfg", path,
                        "--max-steps", "2"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = [float(v) for v in re.findall(r"\[Train Step\] \d+/3: loss=(\S+)", r.stdout)]
    assert len(losses) == 2 and all(np.isfinite(losses)), r.stdout[-2000:]
    assert "DUTS pool: 4 pairs" in r.stdout
    ck = torch.load(os.path.join(res, "model-1.pt"), map_location="cpu", weights_only=True)
    assert ck["step"] == 2 and len([k for k in ck["model"] if k.startswith("model.init_conv_mask.features.")]) > 300
    for name in ("sample-0_2.png", "sample-1.png"):          # B = 2: 2^floor(log2(sqrt 2)) = 1 column, two rows; one channel
        im = Image.open(os.path.join(res, name))
        assert im.mode == "L" and im.size == (192, 384), (name, im.mode, im.size)
    # resume from milestone 1: continues from step 2
    cfg["trainer"].update(resume_milestone=1, test_before=False)
    yaml.safe_dump(cfg, open(path, "w"))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "train_cond_ldm.py"), "--cfg", path,
                        "--max-steps", "1"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "[Train Step] 3/3" in r.stdout and "[Train Step] 1/3" not in r.stdout
    # the sampler on that checkpoint: DUTS-TE in order, one mode-L prediction per photo under its name, PSNR against the resized map
    cfg["data"].update(split="test", augment_horizontal_flip=False)
    yaml.safe_dump(cfg, open(path, "w"))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "sample_cond_ldm.py"), "--cfg", path],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    psnr = re.search(r"PSNR: (-?\d+\.\d+)", r.stdout)
    assert psnr and np.isfinite(float(psnr.group(1))), r.stdout[-1000:]
    names = sorted(os.listdir(os.path.join(res, "png")))
    assert names == ["img_4.png", "img_5.png"], names
    for n in names:
        im = Image.open(os.path.join(res, "png", n))
        assert im.mode == "L" and im.size == (192, 192), (n, im.mode, im.size)
