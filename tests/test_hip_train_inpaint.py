"""GPU: train_cond_ldm.py end to end on a reduced in-painting model -- YAML -> InpaintBatchStream on synthetic data -> optimiser
steps with the built-in Swin-B condition encoder trained along -> masked periodic sample -> checkpoint -> sample_cond_ldm.py on
that checkpoint, which draws a mask per image and writes composites.  Sizes and structure of tests/test_hip_train_cond.py's
super-resolution run: 128x128 images, a ch = 32 first stage (32x32 latents), dim 32."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from sr_data_ref import hash_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reduced_cfg(tmp_path):
    cfg = yaml.load(open(os.path.join(ROOT, "configs/inpainting/celebahq_cond_ddm_const_ldm.yaml")), Loader=yaml.SafeLoader)
    u = cfg["model"]["unet"]
    assert u["cond_encoder"] == "swin_b" and u["train_cond_encoder"] is True and u["dim"] == 96 and u["dim_mults"] == [1, 2, 4, 8]
    assert cfg["data"]["class_name"] == "synthetic" and cfg["data"]["synthetic_of"] == "ddm.data.InpaintDataset"
    assert cfg["data"]["batch_size"] == 48 and cfg["trainer"]["gradient_accumulate_every"] == 2
    assert cfg["trainer"]["lr"] == 4e-5 and cfg["trainer"]["min_lr"] == 4e-6 and cfg["model"]["scale_factor"] == 0.165
    assert cfg["model"]["use_l1"] is True and cfg["model"]["weighting_loss"] is False
    cfg["model"].update(image_size=[128, 128], sampling_timesteps=2)
    cfg["model"]["first_stage"]["ddconfig"].update(ch=32, resolution=[128, 128])
    u.update(dim=32, cond_feature_size=[32, 32])
    cfg["data"].update(image_size=[128, 128], batch_size=2)
    res = str(tmp_path / "run")
    cfg["trainer"].update(results_folder=res, gradient_accumulate_every=2, train_num_steps=3, save_and_sample_every=2, log_freq=1,
                          test_before=True, ema_update_after_step=1, ema_update_every=1, resume_milestone=0)
    cfg["sampler"].update(sample_num=2, cond_encoder="swin_b", use_ema=True, save_masks=True, ckpt_path=os.path.join(res, "model-1.pt"),
                          save_folder=os.path.join(res, "png"))
    return cfg, res


def test_train_and_sample_inpainting_cli_end_to_end(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from PIL import Image
    cfg, res = reduced_cfg(tmp_path)
    path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "train_cond_ldm.py"), "--cfg", path,
                        "--max-steps", "2"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = [float(v) for v in re.findall(r"\[Train Step\] \d+/3: loss=(\S+)", r.stdout)]
    assert len(losses) == 2 and all(np.isfinite(losses)), r.stdout[-2000:]
    lrs = [float(v) for v in re.findall(r"lr=(\S+)", r.stdout)]
    assert lrs[0] == pytest.approx(4e-5 * (1 - 1 / 3) ** 0.96, rel=2e-3)          # the conditional trainer's schedule, the recipe's lr
    ck = torch.load(os.path.join(res, "model-1.pt"), map_location="cpu", weights_only=True)
    assert set(ck) == {"step", "model", "opt", "lr_scheduler", "ema", "scaler"} and ck["step"] == 2
    assert len([k for k in ck["model"] if k.startswith("model.init_conv_mask.features.")]) > 300
    assert os.path.exists(os.path.join(res, "sample-0_2.png")) and os.path.exists(os.path.join(res, "sample-1.png"))
    assert Image.open(os.path.join(res, "sample-1.png")).size == (128, 256)          # B = 2: one column, two rows
    # the sampler on that checkpoint: two known images, a mask drawn for each, composites under the images' names
    x = hash_bytes((2, 128, 128, 3), "inp.sample.pool")
    np.save(tmp_path / "faces.npy", x)
    cfg["data"].update(class_name="ddm.data.InpaintDataset", npy=str(tmp_path / "faces.npy"), split="test")
    yaml.safe_dump(cfg, open(path, "w"))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "sample_cond_ldm.py"), "--cfg", path],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert re.search(r"PSNR: \d+\.\d+", r.stdout), r.stdout[-1000:]
    names = sorted(n for n in os.listdir(os.path.join(res, "png")) if n.endswith(".png"))
    assert names == [f"{0: 010d}.png", f"{1: 010d}.png"], names
    for i, n in enumerate(names):
        out = np.asarray(Image.open(os.path.join(res, "png", n)))
        mask = np.asarray(Image.open(os.path.join(res, "png", "masks", n)))
        assert out.shape == (128, 128, 3) and mask.shape == (128, 128) and set(np.unique(mask).tolist()) <= {0, 255}
        keep = mask == 255
        assert 0 < keep.mean() < 1          # (a fallback mask, all ones, has probability 6e-8)
        assert np.array_equal(out[keep], x[i][keep])          # the kept pixels are the input image's bytes
        assert not np.array_equal(out[~keep], x[i][~keep])    # the holes are the model's
