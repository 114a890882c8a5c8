"""GPU: train_cond_ldm.py end to end on a reduced super-resolution model -- YAML -> SRBatchStream -> optimiser steps with the
built-in Swin-B condition encoder trained along -> checkpoint carrying init_conv_mask.* -> resume -> sample_cond_ldm.py on that
checkpoint with the condition of ddm.data.SRDatasetTest -- and one training step whose batch is checked against the numpy
restatement of ddm.data.SRDataset.  Geometry of test_hip_swin_train.test_train_cond_encoder_wiring scaled to a driver run:
128x128 images, a ch = 32 first stage (32x32 latents), dim 32, 32x32 condition images."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import sr_data_ref as R
from oracle import fill
from parity import close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reduced_cfg(tmp_path):
    cfg = yaml.load(open(os.path.join(ROOT, "configs/super-resolution/div2k_cond_ddm_const_ldm_train.yaml")), Loader=yaml.SafeLoader)
    assert cfg["model"]["unet"]["cond_encoder"] == "swin_b" and cfg["model"]["unet"]["train_cond_encoder"] is True
    assert cfg["data"]["class_name"] == "ddm.data.SRDataset" and not cfg["data"]["img_folder"]
    cfg["model"].update(image_size=[128, 128], sampling_timesteps=2)
    cfg["model"]["first_stage"]["ddconfig"].update(ch=32, resolution=[128, 128])
    cfg["model"]["unet"].update(dim=32)
    npy = str(tmp_path / "hr.npy")
    np.save(npy, R.hash_bytes((6, 160, 144, 3), "sr.train.pool"))
    cfg["data"].update(npy=npy, image_size=[128, 128], batch_size=2)
    res = str(tmp_path / "run")
    cfg["trainer"].update(results_folder=res, gradient_accumulate_every=2, train_num_steps=3, save_and_sample_every=2, log_freq=1,
                          test_before=True, ema_update_after_step=1, ema_update_every=1, resume_milestone=0)
    cfg["sampler"].update(sample_num=1, crop_size=[32, 32], stride=[32, 32], window_batch=0, cond_encoder="swin_b", use_ema=True,
                          ckpt_path=os.path.join(res, "model-1.pt"), save_folder=os.path.join(res, "png"))
    return cfg, res


def test_train_cond_ldm_cli_end_to_end(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cfg, res = reduced_cfg(tmp_path)
    path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_cond_ldm.py"), "--cfg", path, "--max-steps", "2"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = [float(v) for v in re.findall(r"\[Train Step\] \d+/3: loss=(\S+)", r.stdout)]
    assert len(losses) == 2 and all(np.isfinite(losses)), r.stdout[-2000:]
    assert "cond_encoder_weights is not set" in r.stderr          # the reference starts the encoder from ImageNet weights
    lrs = [float(v) for v in re.findall(r"lr=(\S+)", r.stdout)]
    assert lrs[0] == pytest.approx(5e-5 * (1 - 1 / 3) ** 0.96, rel=2e-3)          # no warm-up: lr after step 1 of 3
    ck = torch.load(os.path.join(res, "model-1.pt"), map_location="cpu", weights_only=True)
    assert set(ck) == {"step", "model", "opt", "lr_scheduler", "ema", "scaler"} and ck["step"] == 2
    enc = [k for k in ck["model"] if k.startswith("model.init_conv_mask.features.")]
    assert len(enc) > 300 and "model.init_conv_mask.first_coonv.0.weight" in ck["model"]
    assert all("ema_model." + k in ck["ema"] and "online_model." + k in ck["ema"] for k in enc)
    k = "model.init_conv_mask.features.4.17.mlp.0.weight"
    assert not torch.equal(ck["ema"]["ema_model." + k], torch.zeros_like(ck["ema"]["ema_model." + k]))
    assert os.path.exists(os.path.join(res, "sample-0_2.png")) and os.path.exists(os.path.join(res, "sample-1.png"))
    from PIL import Image
    assert Image.open(os.path.join(res, "sample-1.png")).size == (128, 256)          # B = 2: 2^floor(log2(sqrt 2)) = 1 column, two rows
    # resume from milestone 1: continues from step 2
    cfg["trainer"].update(resume_milestone=1, test_before=False)
    yaml.safe_dump(cfg, open(path, "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_cond_ldm.py"), "--cfg", path, "--max-steps", "1"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "[Train Step] 3/3" in r.stdout and "[Train Step] 1/3" not in r.stdout
    # the sampler on that checkpoint, with the condition the reference's test set makes (160x144 -> 256x256 frame -> 64x64)
    cfg["data"].update(class_name="ddm.data.SRDatasetTest")
    yaml.safe_dump(cfg, open(path, "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sample_cond_ldm.py"), "--cfg", path], capture_output=True, text=True,
                       env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    names = sorted(os.listdir(os.path.join(res, "png")))
    assert names == [f"{0: 010d}.png"], names
    assert Image.open(os.path.join(res, "png", names[0])).size == (144, 160)


def test_training_step_sees_the_reference_batch(tmp_path):
    """One step in process: the batch SRBatchStream makes of injected draws is torch.equal to the batch assembled by hand from
    tests/sr_data_ref.py, and both give the model the same loss (tests/parity.close)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd.ddm.sr_data import SRBatchStream
    from train_uncond_dpm import Cfg, build_model
    gpu = torch.device("cuda:0")
    cfg, _ = reduced_cfg(tmp_path)
    cfg = Cfg(cfg)
    torch.manual_seed(21)
    ldm = build_model(cfg.model).to(gpu).eval()          # (eval: the denoiser's dropout seeds advance from call to call)
    ldm.model.init_conv_mask.train()                     # stochastic depth stays on: its draws come from the seeded device generator
    stream = SRBatchStream(cfg.data, 2, (128, 128), gpu, seed=5)
    idx, top, left, flip = [3, 0], [5, 32], [16, 0], [1, 0]
    batch = stream.next_batch(idx=idx, top=top, left=left, flip=flip)
    x = np.load(cfg.data.npy)
    pairs = [R.sr_pair(x[i], t, l, (128, 128), flip=bool(f)) for i, t, l, f in zip(idx, top, left, flip)]
    hand = {"image": R.to_float(np.stack([p[0] for p in pairs])).to(gpu), "cond": R.to_float(np.stack([p[1] for p in pairs])).to(gpu)}
    assert list(batch) == ["image", "cond"]
    assert torch.equal(batch["image"], hand["image"]) and torch.equal(batch["cond"], hand["cond"])
    ldm.on_train_batch_start(batch)
    t = torch.tensor([0.3, 0.7], device=gpu)
    noise, eps = (fill.hash_tensor((2, 3, 32, 32), f"sr.train.{k}", 1.0).to(gpu) for k in ("noise", "eps"))
    losses = []
    for b in (batch, hand):
        torch.manual_seed(22)
        loss, log = ldm.training_step(b, eps=eps, t=t, noise=noise)
        losses.append(loss.detach())
    assert bool(torch.isfinite(losses[0])) and float(losses[0]) > 0
    close(losses[0], losses[1])
