"""GPU: train_vae.py end to end on the three first-stage recipes (configs/saliency/duts_ae_kl_384x384.yaml -- ONE channel --,
configs/sketch2img/sketchcoco_ae_kl_256x256_d4.yaml, configs/super-resolution/div2k_ae_kl_512x512_d4.yaml), each shrunk to ch 32
at 64x64 with B = 2; the one-channel checkpoint as the first stage of the latent saliency recipe under train_cond_ldm.py; and
train_uncond_ldm.py on a folder of PNGs through ddm.data.ImageDataset.  Every driver runs as a child process."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_KEYS = {"total_loss", "logvar", "kl_loss", "nll_loss", "rec_loss", "d_weight", "disc_factor", "g_loss", "disc_loss", "logits_real",
            "logits_fake"}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def run(script, path, steps):
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, script), "--cfg", path, "--max-steps", str(steps)],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def shrunk_vae_cfg(rel, tmp_path, steps):
    cfg = yaml.load(open(os.path.join(ROOT, "configs", rel)), Loader=yaml.SafeLoader)
    cfg["model"]["ddconfig"].update(ch=32, resolution=[64, 64])
    cfg["model"]["lossconfig"]["disc_start"] = 2
    cfg["data"].update(image_size=[64, 64], batch_size=2)
    res = str(tmp_path / "run")
    cfg["trainer"].update(results_folder=res, train_num_steps=steps, save_and_sample_every=3, log_freq=1, ema_update_after_step=1,
                          ema_update_every=1)
    path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    return cfg, path, res


def vae_logs(stdout, total):
    lines = re.findall(rf"\[Train Step\] (\d+)/{total}: (.*) lr=", stdout)
    logs = [dict((kv.split("=")[0], float(kv.split("=")[1])) for kv in l[1].split()) for l in lines]
    assert all(set(lg) == LOG_KEYS and all(math.isfinite(v) for v in lg.values()) for lg in logs), logs
    return [int(l[0]) for l in lines], logs


def test_one_channel_first_stage_trains_and_serves_the_latent_recipe(gpu, tmp_path):
    """train_vae.py on the shrunk DUTS first-stage YAML: 3 steps (disc_start 2), finite logs, model-1.pt, a mode-L sample-1.png;
    the checkpoint is then model.first_stage.ckpt_path of a shrunk configs/saliency/duts_cond_ddm_const_ldm.yaml, and
    train_cond_ldm.py takes one step with it."""
    from PIL import Image
    cfg, path, res = shrunk_vae_cfg("saliency/duts_ae_kl_384x384.yaml", tmp_path, 3)
    assert cfg["model"]["ddconfig"]["in_channels"] == 1 and cfg["data"]["synthetic_of"] == "ddm.data.DUTSDataset"
    out = run("train_vae.py", path, 3)
    assert "DUTS map pool: 32 images of 1 channel(s)" in out and "MiB resident in device memory" in out
    steps, logs = vae_logs(out, 3)
    assert steps == [0, 1, 2], out[-2000:]
    assert [lg["disc_factor"] for lg in logs] == [0.0, 0.0, 1.0] and logs[0]["disc_loss"] == 0.0 and logs[2]["disc_loss"] > 0.0
    ck_path = os.path.join(res, "model-1.pt")
    ck = torch.load(ck_path, map_location="cpu", weights_only=True)
    assert ck["step"] == 3 and tuple(ck["model"]["encoder.conv_in.weight"].shape) == (32, 1, 3, 3)
    assert tuple(ck["model"]["decoder.conv_out.weight"].shape) == (1, 32, 3, 3)
    assert tuple(ck["model"]["loss.discriminator.main.0.weight"].shape) == (64, 1, 4, 4)
    im = Image.open(os.path.join(res, "sample-1.png"))
    assert im.mode == "L" and im.size == (128, 64), (im.mode, im.size)          # two reconstructions side by side
    # ... as the first stage of the latent saliency recipe
    ldm = yaml.load(open(os.path.join(ROOT, "configs/saliency/duts_cond_ddm_const_ldm.yaml")), Loader=yaml.SafeLoader)
    ldm["model"].update(image_size=[192, 192], sampling_timesteps=2)
    ldm["model"]["first_stage"]["ddconfig"].update(ch=32, resolution=[192, 192])
    ldm["model"]["first_stage"]["ckpt_path"] = ck_path
    ldm["model"]["unet"].update(dim=32, cond_feature_size=[48, 48])
    ldm["data"].update(image_size=[192, 192], batch_size=2)
    res2 = str(tmp_path / "ldm")
    ldm["trainer"].update(results_folder=res2, gradient_accumulate_every=1, train_num_steps=2, save_and_sample_every=1, log_freq=1,
                          test_before=False, ema_update_after_step=1, ema_update_every=1, resume_milestone=0)
    path2 = str(tmp_path / "ldm.yaml")
    yaml.safe_dump(ldm, open(path2, "w"))
    out = run("train_cond_ldm.py", path2, 1)
    assert f"Restored from {ck_path}" in out
    losses = [float(v) for v in re.findall(r"\[Train Step\] \d+/2: loss=(\S+)", out)]
    assert len(losses) == 1 and math.isfinite(losses[0]), out[-2000:]
    saved = torch.load(os.path.join(res2, "model-1.pt"), map_location="cpu", weights_only=True)["model"]
    assert torch.equal(saved["first_stage_model.decoder.conv_out.weight"], ck["ema"]["ema_model.decoder.conv_out.weight"])


@pytest.mark.parametrize("rel,pool", [("sketch2img/sketchcoco_ae_kl_256x256_d4.yaml", "sketch photo pool: 32 images of 3 channel(s)"),
                                      ("super-resolution/div2k_ae_kl_512x512_d4.yaml", None)])
def test_three_channel_first_stage_recipes_take_a_step(gpu, tmp_path, rel, pool):
    """One step each of the shrunk sketch (photos through adm_image_resize_batch) and DIV2K (HR crops of the SR stream) YAMLs."""
    cfg, path, _ = shrunk_vae_cfg(rel, tmp_path, 2)
    out = run("train_vae.py", path, 1)
    steps, logs = vae_logs(out, 2)
    assert steps == [0] and logs[0]["nll_loss"] > 0, out[-2000:]
    if pool:
        assert pool in out


def test_uncond_ldm_trains_on_an_image_folder(gpu, tmp_path):
    """train_uncond_ldm.py --max-steps 1 on eight small PNGs of different sizes through ddm.data.ImageDataset + img_folder."""
    import numpy as np
    from PIL import Image
    from sr_data_ref import hash_bytes
    folder = tmp_path / "faces"
    folder.mkdir()
    for i in range(8):
        Image.fromarray(hash_bytes((40 + 5 * i, 70 - 3 * i, 3), f"cli.face{i}")).save(folder / f"{i}.png")
    cfg = yaml.load(open(os.path.join(ROOT, "configs/celebahq/celeb_uncond_ddm_const2_unet_ldm.yaml")), Loader=yaml.SafeLoader)
    cfg["model"].update(image_size=[64, 64], default_scale=False, scale_factor=1.0)
    cfg["model"]["first_stage"]["ddconfig"].update(ch=32, resolution=[64, 64])
    cfg["model"]["unet"].update(img_resolution=16, model_channels=64, num_blocks=1, attn_resolutions=[8])
    cfg["data"] = dict(class_name="ddm.data.ImageDataset", img_folder=str(folder), image_size=[64, 64], batch_size=4,
                       augment_horizontal_flip=True)
    res = str(tmp_path / "run")
    cfg["trainer"].update(results_folder=res, train_num_steps=2, save_and_sample_every=1, log_freq=1, test_before=False,
                          gradient_accumulate_every=2, ema_update_after_step=1, ema_update_every=1)
    path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    out = run("train_uncond_ldm.py", path, 1)
    assert "image pool: 8 images of 3 channel(s)" in out and "USING STD-RESCALING" in out
    losses = [float(v) for v in re.findall(r"\[Train Step\] \d+/2: loss=(\S+)", out)]
    assert len(losses) == 1 and np.isfinite(losses[0]), out[-2000:]
    assert torch.load(os.path.join(res, "model-1.pt"), map_location="cpu", weights_only=True)["step"] == 1
