#!/usr/bin/env python3
"""Sampler of the conditional PIXEL-SPACE saliency model trained by train_cond_dpm.py (configs/saliency/
duts_cond_ddm_const_dpm_sample.yaml).  The reference has no such script: its sample_cond_ldm.py asserts ``ldm`` (:58).

``python sample_cond_dpm.py --cfg <yaml>`` builds unet.cond_unet.Unet + ddm.ddm_const.DDPM from the YAML, loads ``sampler.ckpt_path``
(EMA weights when ``sampler.use_ema``), walks ``split: test`` of ddm.data.DUTSDataset in order (the stream of sample_cond_ldm.py: photo
and map resized to the model's resolution on the device) and calls ``sample(cond=photos)`` once per ``sampler.batch_size`` photos -- no
windows, the condition encoder run once per call.  Each one-channel prediction is written as a mode-L ``<photo name>.png`` and the
PSNR against the resized map is printed.  ``sampler.cal_saliency: True`` (off by default; ``sampler.saliency_normalize``, default True) also
scores each prediction's bytes against the resized map's bytes with adm_amd.metrics.saliency (MAE, F-, S- and E-measure): printed at the end
and written to ``<save_folder>/saliency_metrics.json``.  Every rank handles a disjoint share of the photos; no collectives.
"""
import os

import torch

from adm_amd.ddm.datasets import DATASETS, DUTS_CLASSES, dataset_of
from sample_cond_ldm import DatasetCondStream, load_checkpoint, report_saliency, saliency_scorer, save_prediction, start
from train_uncond_dpm import build_model


def batches(stream, size):
    """Groups the one-photo items of DatasetCondStream into batches of up to `size`."""
    items = []
    for item in stream:
        items.append(item)
        if len(items) == size:
            yield items
            items = []
    if items:
        yield items


def check_dataset(data_cfg):
    if dataset_of(data_cfg) != DUTS_CLASSES[0]:
        raise NotImplementedError(f"data.class_name {data_cfg.get('class_name')!r}: the pixel-space conditional sampler reads "
                                  "ddm.data.DUTSDataset")


def main():
    args, cfg, world, rank, device = start("conditional pixel-space sampler (MI355X hot path)")
    mc, s = cfg.model, cfg.sampler
    if mc.get("ldm") or mc.get("first_stage"):
        raise ValueError("sample_cond_dpm.py samples pixel-space models (ldm: False, no first_stage); use sample_cond_ldm.py")
    saliency_score = saliency_scorer(cfg.data, s)          # (first: the key on another data set is refused by its own name)
    check_dataset(cfg.data)
    dpm = build_model(mc).to(device).eval()
    if not isinstance(getattr(dpm.model, "init_conv_mask", None), torch.nn.Module):
        raise ValueError("the unet section must build the condition encoder (unet.cond_encoder: swin_b): its weights come from the checkpoint")
    load_checkpoint(dpm, s, args.random_init, device, "{path} lacks {n} of the condition encoder's tensors (first: {first})")
    os.makedirs(s.save_folder, exist_ok=True)
    n_total = int(s.sample_num) if args.max_images is None else min(int(s.sample_num), args.max_images)
    per_rank = n_total // world
    size = tuple(cfg.data.get("image_size") or mc.image_size)
    if size != tuple(mc.image_size):
        raise ValueError(f"data.image_size {size} must equal model.image_size {tuple(mc.image_size)}: there are no windows")
    stream = DatasetCondStream(DATASETS[DUTS_CLASSES[0]], cfg.data, per_rank, size, device, seed=2000 + rank,
                               want_u8=saliency_score is not None)
    psnr, done = 0.0, 0
    for items in batches(stream, max(int(s.get("batch_size", 1)), 1)):
        cond = torch.cat([it["cond"] for it in items])
        image = (torch.cat([it["image"] for it in items]) + 1) * 0.5
        pred = dpm.sample(cond=cond).to(torch.float32)
        if saliency_score is not None:          # one launch per batch; the tables stay on the device
            saliency_score.add(pred[:, :1].contiguous(), torch.cat([it["image_u8"] for it in items]))
        for k, it in enumerate(items):
            psnr += float(-10.0 * torch.log10(torch.mean((pred[k] - image[k]) ** 2)))
            save_prediction(pred[k, :1], s.save_folder, it["img_name"], world, rank * per_rank + done, gray=True)
            done += 1
    torch.cuda.synchronize()
    print(f"rank {rank}: {done} images; PSNR: {psnr / max(done, 1):.2f}")
    if saliency_score is not None:
        report_saliency(saliency_score, s.save_folder, world, rank)


if __name__ == "__main__":
    main()
