#!/usr/bin/env python3
"""Cost of making the super-resolution training batches on one MI355X, next to the training step they feed.

  python tools/sr_data_cost.py --out profiles/sr_data_cost.json

Three figures:
  * milliseconds per batch of adm_sr_batch at the recipe's shape (B = 16, 512x512 crops, /4 bicubic; HIP events after warm-up,
    median (min, max) of --reps launches), with and without the draws made on the device by SRBatchStream;
  * the same batch made by PIL on this host's CPU in one process (crop -> Image.resize -> flip -> uint8 -> float, the steps of
    ddm.data.SRDataset: the reference's path, which it spreads over data.num_workers processes); null when PIL is not importable;
  * the SR training step measured in the same process: configs/super-resolution/div2k_cond_ddm_const_ldm_train.yaml with
    data.class_name: synthetic -- the batch from the stream, forward, backward through the denoiser and the Swin-B encoder,
    gradient_accumulate_every micro-batches, the fused optimiser step.
The weights are the default initialisation and the images U(0,255) (the cost depends on neither)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)]


def pil_batch_ms(images, draws, size, down, reps):
    try:
        from PIL import Image
    except ImportError:
        return None
    H, W = size
    pil = [Image.fromarray(a) for a in images]
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = []
        for i, t, l, f in draws:
            crop = pil[i].crop((l, t, l + W, t + H))
            mask = crop.copy().resize((W // down, H // down), resample=Image.BICUBIC)
            if f:
                crop, mask = crop.transpose(Image.FLIP_LEFT_RIGHT), mask.transpose(Image.FLIP_LEFT_RIGHT)
            out.append([torch.from_numpy(np.asarray(x).copy()).permute(2, 0, 1).float().div(255) * 2 - 1 for x in (crop, mask)])
        torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])
        ms.append((time.perf_counter() - t0) * 1e3)
    return [round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=4, help="training steps timed (after --warmup steps)")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from adm_amd import hip
    from adm_amd.ddm.sr_data import SRBatchStream, sr_batch
    from train_uncond_dpm import Cfg, build_model
    hip.lib()
    dev = torch.device("cuda", 0)
    cfg = yaml.load(open(os.path.join(ROOT, "configs/super-resolution/div2k_cond_ddm_const_ldm_train.yaml")), Loader=yaml.SafeLoader)
    cfg["data"].update(class_name="synthetic", batch_size=args.batch)
    cfg = Cfg(cfg)
    size = tuple(cfg.data.image_size)
    stream = SRBatchStream(cfg.data, args.batch, size, dev, seed=1)
    draws = stream.draw()
    res = {"what": "super-resolution training batches (adm_sr_batch) on one MI355X; ms = median (min, max)",
           "batch": args.batch, "crop": list(size), "down": stream.down, "filter": stream.filter, "reps": args.reps,
           "pool_images": stream.pool.n, "pool_image_size": stream.pool.hw[0].tolist()}
    res["kernel_ms_per_batch"] = timed(lambda: sr_batch(stream.pool, stream.rs, *draws), args.warmup, args.reps)
    res["stream_ms_per_batch_with_device_draws"] = timed(lambda: next(stream), args.warmup, args.reps)
    out_bytes = args.batch * 3 * 4 * (size[0] * size[1] + size[0] * size[1] // stream.down ** 2)
    res["output_MB_per_batch"] = round(out_bytes / 1e6, 2)
    n = stream.pool.n
    h, w = stream.pool.hw[0].tolist()
    host = stream.pool.flat[:n * h * w * 3].reshape(n, h, w, 3).cpu().numpy()
    d = [tuple(int(v[k]) for v in draws) for k in range(args.batch)]
    res["pil_ms_per_batch_one_process"] = pil_batch_ms(host, d, size, stream.down, max(3, args.reps // 4))
    res["host_cpus_visible"] = os.cpu_count()
    if not args.skip_train:
        from adm_amd.optim import BucketedGradReducer, FlatParams, FusedAdamWEMA, lr_lambda_cond
        t = cfg.trainer
        torch.manual_seed(7)
        ldm = build_model(cfg.model).to(dev).train()
        flat = FlatParams(ldm)
        reducer = BucketedGradReducer(flat)
        opt = FusedAdamWEMA(flat, lr=float(t.lr), weight_decay=1e-2, max_norm=1.0, ema=True)
        accum = int(t.gradient_accumulate_every)
        ldm.on_train_batch_start(next(stream))

        def step(it):
            flat.zero_grad()
            for _ in range(accum):
                loss, _ = ldm.training_step(next(stream))
                (loss / accum).backward()
            reducer.finish()
            opt.step(lr=float(t.lr) * lr_lambda_cond(it, float(t.lr), float(t.min_lr), int(t.train_num_steps)), grad_scale=1.0,
                     ema_decay=None)
            return loss

        for it in range(args.warmup):
            step(it)
        torch.cuda.synchronize()
        ms = []
        for it in range(args.steps):
            t0 = time.perf_counter()
            loss = step(args.warmup + it)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        assert bool(torch.isfinite(loss))
        res["train_step_ms"] = [round(statistics.median(ms), 2), round(min(ms), 2), round(max(ms), 2)]
        res["train_step"] = {"micro_batches": accum, "images_per_step": accum * args.batch, "steps_timed": args.steps,
                             "model": "ddm_const.LatentDiffusion, KL-f4 first stage, unet.cond_unet.Unet dim 128, Swin-B encoder trained"}
        res["batches_share_of_step_percent"] = round(100.0 * accum * res["stream_ms_per_batch_with_device_draws"][0] / res["train_step_ms"][0], 3)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
