#!/usr/bin/env python3
"""Cost of making the in-painting training batches on one MI355X, next to the training step they feed.

  python tools/inpaint_data_cost.py --out profiles/inpaint_data_cost.json

Figures (ms = median (min, max)):
  * adm_inpaint_batch alone at the recipe's shape (B = 48, 256x256; HIP events after warm-up, --reps launches), adm_inpaint_masks
    alone, and the stream's whole batch with the draws made on the device;
  * the same batch on this host's CPU in one process: the primitive lists from the NumPy restatement (tests/inpaint_ref.py), the
    masks drawn with PIL through the calls ddm.data.RandomBrush makes, mask * image in torch -- the reference's path, which it
    spreads over data.num_workers processes; null when PIL is not importable;
  * the training step measured in the same process: configs/inpainting/celebahq_cond_ddm_const_ldm.yaml on synthetic data -- the
    batch from the stream, forward, backward through the denoiser and the Swin-B encoder, gradient_accumulate_every micro-batches,
    the fused optimiser step.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sr_data_cost import timed  # noqa: E402


def host_batch_ms(images, idx, flip, u, z, S, reps):
    try:
        from PIL import Image, ImageDraw
    except ImportError:
        return None
    import inpaint_ref as R
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = []
        for b in range(len(idx)):
            _, c, _ = R.geometry(u[b], z[b], S)
            mask = np.ones((S, S), np.uint8)
            for _, x, y, w, h in c["raw_rects"]:
                mask[max(y, 0): min(y + h, S), max(x, 0): min(x + w, S)] = 0
            im = Image.new("L", (S, S), 0)
            for vertex, width in c["strokes"]:
                draw = ImageDraw.Draw(im)
                draw.line(vertex, fill=1, width=width)
                for v in vertex:
                    draw.ellipse((v[0] - width // 2, v[1] - width // 2, v[0] + width // 2, v[1] + width // 2), fill=1)
            brush = np.asarray(im, np.uint8)
            if c["flips"][0]:
                brush = np.flip(brush, 0)
            if c["flips"][1]:
                brush = np.flip(brush, 1)
            m = torch.from_numpy(np.logical_and(mask, 1 - brush)[None].astype(np.float32))
            a = images[idx[b]][:, ::-1] if flip[b] else images[idx[b]]
            img = torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1).float().div(255)
            out.append((img * 2 - 1, (m * img) * 2 - 1, m))
        [torch.stack([o[k] for o in out]) for k in range(3)]
        ms.append((time.perf_counter() - t0) * 1e3)
    return [round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=4, help="training steps timed (after --warmup steps)")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from adm_amd import hip
    from adm_amd.ddm.inpaint_data import InpaintBatchStream, inpaint_batch, inpaint_masks
    from train_uncond_dpm import Cfg, build_model
    hip.lib()
    dev = torch.device("cuda", 0)
    cfg = yaml.load(open(os.path.join(ROOT, "configs/inpainting/celebahq_cond_ddm_const_ldm.yaml")), Loader=yaml.SafeLoader)
    cfg["data"].update(class_name="synthetic", synthetic_of="ddm.data.InpaintDataset", batch_size=args.batch)
    cfg = Cfg(cfg)
    S = int(cfg.data.image_size[0])
    stream = InpaintBatchStream(cfg.data, args.batch, (S, S), dev, seed=1)
    idx, flip, u, z = stream.draw()
    prims = inpaint_masks(u, z, S)
    res = {"what": "in-painting training batches (adm_inpaint_masks + adm_inpaint_batch) on one MI355X; ms = median (min, max)",
           "batch": args.batch, "size": S, "reps": args.reps, "pool_images": stream.pool.n}
    res["batch_kernel_ms"] = timed(lambda: inpaint_batch(stream.pool, idx, flip, prims, S), args.warmup, args.reps)
    res["masks_kernel_ms"] = timed(lambda: inpaint_masks(u, z, S), args.warmup, args.reps)
    res["stream_ms_per_batch_with_device_draws"] = timed(lambda: next(stream), args.warmup, args.reps)
    res["output_MB_per_batch"] = round(args.batch * 7 * 4 * S * S / 1e6, 2)
    host = stream.pool.flat[:stream.pool.n * S * S * 3].reshape(stream.pool.n, S, S, 3).cpu().numpy()
    res["host_numpy_pil_ms_per_batch_one_process"] = host_batch_ms(host, idx.tolist(), flip.tolist(), u.cpu().numpy(), z.cpu().numpy(), S,
                                                                   max(3, args.reps // 4))
    res["host_cpus_visible"] = os.cpu_count()
    res["fallbacks"] = int(stream.fallbacks)
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
                             "model": "ddm_const.LatentDiffusion, KL-f4 first stage, unet.cond_unet.Unet dim 96 x (1,2,4,8), Swin-B encoder trained"}
        res["batches_share_of_step_percent"] = round(100.0 * accum * res["stream_ms_per_batch_with_device_draws"][0] / res["train_step_ms"][0], 3)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
