#!/usr/bin/env python3
"""Sampler of the conditional PIXEL-SPACE saliency model trained by train_cond_dpm.py (configs/saliency/
duts_cond_ddm_const_dpm_sample.yaml).  The reference has no such script: its sample_cond_ldm.py asserts ``ldm`` (:58).

``python sample_cond_dpm.py --cfg <yaml>`` builds unet.cond_unet.Unet + ddm.ddm_const.DDPM from the YAML, loads ``sampler.ckpt_path``
(EMA weights when ``sampler.use_ema``), walks ``split: test`` of ddm.data.DUTSDataset in order (the stream of sample_cond_ldm.py: photo
and map resized to the model's resolution on the device) and calls ``sample(cond=photos)`` once per ``sampler.batch_size`` photos -- no
windows, the condition encoder run once per call.  Each one-channel prediction is written as a mode-L ``<photo name>.png`` and the
PSNR against the resized map is printed.  Every rank handles a disjoint share of the photos; no collectives.
"""
import argparse
import os

import torch
import yaml

from sample_cond_ldm import DUTS_CLASSES, DUTSCondStream
from sample_uncond import load_weights
from train_uncond_dpm import Cfg, build_model


def batches(stream, size):
    """Groups the one-photo items of DUTSCondStream into batches of up to `size`."""
    items = []
    for item in stream:
        items.append(item)
        if len(items) == size:
            yield items
            items = []
    if items:
        yield items


def main():
    ap = argparse.ArgumentParser(description="conditional pixel-space sampler (MI355X hot path)")
    ap.add_argument("--cfg", required=True)
    ap.add_argument("--max-images", type=int, default=None)
    ap.add_argument("--random-init", action="store_true", help="smoke runs: sample without loading a checkpoint")
    args = ap.parse_args()
    with open(args.cfg) as f:
        cfg = Cfg(yaml.load(f, Loader=yaml.SafeLoader))
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.manual_seed(42 + rank)
    mc, s = cfg.model, cfg.sampler
    if mc.get("ldm") or mc.get("first_stage"):
        raise ValueError("sample_cond_dpm.py samples pixel-space models (ldm: False, no first_stage); use sample_cond_ldm.py")
    cls = cfg.data.get("class_name")
    if not (cls in DUTS_CLASSES or (cls == "synthetic" and cfg.data.get("synthetic_of") in DUTS_CLASSES)):
        raise NotImplementedError(f"data.class_name {cls!r}: the pixel-space conditional sampler reads ddm.data.DUTSDataset")
    dpm = build_model(mc).to(device).eval()
    if not isinstance(getattr(dpm.model, "init_conv_mask", None), torch.nn.Module):
        raise ValueError("the unet section must build the condition encoder (unet.cond_encoder: swin_b): its weights come from the checkpoint")
    if s.get("ckpt_path") and not args.random_init:
        if not os.path.exists(s.ckpt_path):
            raise FileNotFoundError(f"sampler.ckpt_path {s.ckpt_path} does not exist (pass --random-init for a smoke run)")
        missing, _ = load_weights(dpm, s.ckpt_path, s.get("use_ema", True), device)
        lost = [k for k in missing if ".init_conv_mask." in k and ".init_conv_mask.norm." not in k and ".init_conv_mask.head." not in k]
        if lost:
            raise RuntimeError(f"{s.ckpt_path} lacks {len(lost)} of the condition encoder's tensors (first: {lost[0]})")
    elif not args.random_init:
        raise ValueError("sampler.ckpt_path is empty (pass --random-init for a smoke run)")
    os.makedirs(s.save_folder, exist_ok=True)
    from PIL import Image
    n_total = int(s.sample_num) if args.max_images is None else min(int(s.sample_num), args.max_images)
    per_rank = n_total // world
    size = tuple(cfg.data.get("image_size") or mc.image_size)
    if size != tuple(mc.image_size):
        raise ValueError(f"data.image_size {size} must equal model.image_size {tuple(mc.image_size)}: there are no windows")
    stream = DUTSCondStream(cfg.data, per_rank, size, device, seed=2000 + rank)
    psnr, done = 0.0, 0
    for items in batches(stream, max(int(s.get("batch_size", 1)), 1)):
        cond = torch.cat([it["cond"] for it in items])
        image = (torch.cat([it["image"] for it in items]) + 1) * 0.5
        pred = dpm.sample(cond=cond).to(torch.float32)
        for k, it in enumerate(items):
            psnr += float(-10.0 * torch.log10(torch.mean((pred[k] - image[k]) ** 2)))
            arr = (pred[k, 0].clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
            name = it["img_name"] if world == 1 else f"{rank * per_rank + done: 010d}.png"
            Image.fromarray(arr).save(os.path.join(s.save_folder, name))
            done += 1
    torch.cuda.synchronize()
    print(f"rank {rank}: {done} images; PSNR: {psnr / max(done, 1):.2f}")


if __name__ == "__main__":
    main()
