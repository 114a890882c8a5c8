#!/usr/bin/env python3
"""Cost of the depth recipe's own pieces on one MI355X, next to the training step and the sampled frame they serve.

  python tools/depth_data_cost.py --out profiles/depth_data_cost.json

Figures (ms = median (min, max)):
  * adm_depth_batch alone at the recipe's shape (B = 8, 320x320 crops of 426x560 boxed frames, the synthetic pool; HIP events after
    warm-up, --reps launches), the depth plane alone (the first-stage form), and the stream's whole batch with its draws made on the
    device;
  * the same batch on this host's CPU in one process with PIL itself through the calls ddm.data.NYUDv2DepthDataset makes (the two
    crops, the flip, np.array, ToTensor, the float maps) -- the reference's path, which it spreads over dataloader workers;
  * the training step measured in the same process: configs/depth_estimation/nyud_cond_ddm_const_ldm.yaml on synthetic data -- the
    batch from the stream, forward, backward through the denoiser and the Swin-B encoder, gradient_accumulate_every micro-batches,
    the fused optimiser step -- and the batches' share of it;
  * adm_depth_metrics on one 426x560 frame and on a batch of 8;
  * one sampled frame of configs/depth_estimation/nyud_cond_ddm_const_ldm_sample.yaml: 2 x 3 windows of 320x320, each twice
    (flip_test), 10 steps each, random weights.
The weights are the default initialisation and the data U(0,255) / U(0,10000) (the cost depends on neither)."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sr_data_cost import timed  # noqa: E402


def median3(ms):
    return [round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)]


def host_pairs(pool, idx):
    """The pool's pairs idx, read back to the host as (uint8 [h,w,3], uint16 [h,w])."""
    rgb, d16 = pool.rgb.cpu().numpy(), pool.depth.cpu().numpy().view("<u2")
    ro, do = pool.rgb_off.cpu().numpy(), pool.depth_off.cpu().numpy()
    out = []
    for n in idx:
        h, w = (int(v) for v in pool.hw_host[n])
        out.append((rgb[ro[n]:ro[n] + h * w * 3].reshape(h, w, 3), d16[do[n] // 2:do[n] // 2 + h * w].reshape(h, w).astype(np.uint16)))
    return out


def host_pil_ms(pairs, box, draws, size, reps):
    from PIL import Image
    H, W = size
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        rgbs, depths = [], []
        for (p, d), t, l, f in zip(pairs, *draws):
            rgb, depth = Image.fromarray(p).crop(box), Image.fromarray(d).crop(box)
            rgb, depth = rgb.crop((l, t, l + W, t + H)), depth.crop((l, t, l + W, t + H))
            if f:
                rgb, depth = rgb.transpose(Image.FLIP_LEFT_RIGHT), depth.transpose(Image.FLIP_LEFT_RIGHT)
            rgbs.append(torch.from_numpy(np.asarray(rgb)).permute(2, 0, 1).float().div(255) * 2 - 1)
            depths.append((torch.from_numpy(np.array(depth).astype(np.float32)) / 10000)[None] * 2 - 1)
        torch.stack(rgbs), torch.stack(depths)
        ms.append((time.perf_counter() - t0) * 1e3)
    return median3(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=4, help="training steps timed (after --warmup steps)")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--skip-sample", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from adm_amd import hip
    from adm_amd.ddm.depth_data import DepthBatchStream, depth_batch
    from adm_amd.metrics.depth import depth_sums
    from train_uncond_dpm import Cfg, build_model
    hip.lib()
    dev = torch.device("cuda", 0)
    load = lambda n: yaml.load(open(os.path.join(ROOT, "configs", "depth_estimation", n)), Loader=yaml.SafeLoader)
    cfg = load("nyud_cond_ddm_const_ldm.yaml")
    cfg["data"].update(batch_size=args.batch)
    cfg = Cfg(cfg)
    size = (int(cfg.data.image_size[0]), int(cfg.data.image_size[1]))
    stream = DepthBatchStream(cfg.data, args.batch, size, dev, seed=1)
    idx, top, left, flip = stream.draw()
    res = {"what": "depth training batches (adm_depth_batch), score (adm_depth_metrics), step and sampled frame on one MI355X; "
                   "ms = median (min, max)", "batch": args.batch, "size": list(size), "reps": args.reps, "pool_pairs": stream.pool.n,
           "pool_bytes": stream.pool.nbytes, "frame_sizes": sorted({(int(h), int(w)) for h, w in stream.pool.hw_host}),
           "border_crop": list(stream.box)}
    res["batch_kernel_ms"] = timed(lambda: depth_batch(stream.pool, idx, top, left, flip, size), args.warmup, args.reps)
    res["depth_plane_only_ms"] = timed(lambda: depth_batch(stream.pool, idx, top, left, flip, size, cond=False), args.warmup, args.reps)
    res["stream_ms_per_batch_with_device_draws"] = timed(lambda: next(stream), args.warmup, args.reps)
    res["output_MB_per_batch"] = round(args.batch * 4 * 4 * size[0] * size[1] / 1e6, 2)
    res["source_MB_per_batch"] = round(args.batch * 5 * size[0] * size[1] / 1e6, 2)
    draws = tuple(v.tolist() for v in (top, left, flip))
    res["host_pil_ms_per_batch_one_process"] = host_pil_ms(host_pairs(stream.pool, idx.tolist()), stream.box, draws, size,
                                                           max(3, args.reps // 4))
    res["host_cpus_visible"] = os.cpu_count()
    fh, fw = stream.pool.frame
    for B in (1, args.batch):
        g = torch.rand(B, 1, fh, fw, device=dev)
        p = (g * torch.exp(0.25 * torch.randn_like(g))).contiguous()
        res[f"metrics_ms_B{B}_{fh}x{fw}"] = timed(lambda: depth_sums(p, g), args.warmup, args.reps)
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
                             "model": "ddm_const.LatentDiffusion, one-channel KL-f4 first stage at 320x320, unet.cond_unet.Unet dim 128 x "
                                      "(1,2,4,4), Swin-B encoder trained"}
        res["batches_share_of_step_percent"] = round(100.0 * accum * res["stream_ms_per_batch_with_device_draws"][0] / res["train_step_ms"][0], 3)
        del ldm, flat, reducer, opt
        torch.cuda.empty_cache()
    if not args.skip_sample:
        import sample_cond_ldm as S
        scfg = Cfg(load("nyud_cond_ddm_const_ldm_sample.yaml"))
        torch.manual_seed(8)
        ldm = build_model(scfg.model).to(dev).eval()
        test = DepthBatchStream(scfg.data, 1, size, dev, seed=2)
        crop, stride = tuple(scfg.sampler.crop_size), tuple(scfg.sampler.stride)
        wins = S.slide_windows(fh, fw, crop, stride)

        def frame():
            with torch.no_grad():
                return S.predict_slide(ldm, scfg.sampler, next(test), crop, stride)

        for _ in range(max(1, args.warmup // 2)):
            pred = frame()
        torch.cuda.synchronize()
        ms = []
        for _ in range(max(2, args.steps // 2)):
            t0 = time.perf_counter()
            pred = frame()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        assert tuple(pred.shape) == (1, 1, fh, fw) and bool(torch.isfinite(pred).all())
        res["sampled_frame_ms"] = [round(statistics.median(ms), 1), round(min(ms), 1), round(max(ms), 1)]
        res["sampled_frame"] = {"frame": [fh, fw], "windows": len(wins), "flip_test": bool(scfg.sampler.flip_test),
                                "samples": len(wins) * (2 if scfg.sampler.flip_test else 1),
                                "sampling_timesteps": int(scfg.model.sampling_timesteps), "frames_timed": len(ms)}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
