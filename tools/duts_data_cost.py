#!/usr/bin/env python3
"""Cost of making the saliency training batches on one MI355X, next to the training step they feed.

  python tools/duts_data_cost.py --out profiles/duts_data_cost.json

Figures (ms = median (min, max)):
  * adm_pair_resize_batch alone at the recipe's shape (B = 8, 384x384, the synthetic pool's ragged sources; HIP events after
    warm-up, --reps launches), and the stream's whole batch with the draws made on the device;
  * the same batch on this host's CPU in one process: the NumPy restatement (tests/duts_data_ref.py) and PIL itself through the
    calls ddm.data.DUTSDataset makes (Image.resize of photo and map, the flip, ToTensor, *2-1) -- the reference's path, which it
    spreads over dataloader workers; null when PIL is not importable;
  * the training step measured in the same process: configs/saliency/duts_cond_ddm_const_ldm.yaml on synthetic data -- the batch
    from the stream, forward, backward through the denoiser and the Swin-B encoder, gradient_accumulate_every micro-batches, the
    fused optimiser step.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sr_data_cost import timed  # noqa: E402


def median3(ms):
    return [round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)]


def host_pairs(pool, idx):
    """The pool's pairs idx, read back to the host as uint8 arrays."""
    rgb, gray, hw = pool.rgb.cpu().numpy(), pool.gray.cpu().numpy(), pool.hw_host[0]
    ro, go = pool.rgb_off.cpu().numpy(), pool.gray_off.cpu().numpy()
    out = []
    for n in idx:
        h, w = int(hw[n, 0]), int(hw[n, 1])
        out.append((rgb[ro[n]:ro[n] + h * w * 3].reshape(h, w, 3), gray[go[n]:go[n] + h * w].reshape(h, w)))
    return out


def host_numpy_ms(pairs, flip, size, reps):
    import duts_data_ref as R
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = [R.duts_pair(p, m, size, flip=bool(f)) for (p, m), f in zip(pairs, flip)]
        R.to_float(np.stack([o[0] for o in out])), R.gray_to_float(np.stack([o[1] for o in out]))
        ms.append((time.perf_counter() - t0) * 1e3)
    return median3(ms)


def host_pil_ms(pairs, flip, size, reps):
    try:
        from PIL import Image
    except ImportError:
        return None
    H, W = size
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        rgbs, gts = [], []
        for (p, m), f in zip(pairs, flip):
            rgb, gt = Image.fromarray(p).resize((W, H), Image.BILINEAR), Image.fromarray(m).resize((W, H), Image.BILINEAR)
            if f:
                rgb, gt = rgb.transpose(Image.FLIP_LEFT_RIGHT), gt.transpose(Image.FLIP_LEFT_RIGHT)
            rgbs.append(torch.from_numpy(np.asarray(rgb)).permute(2, 0, 1).float().div(255) * 2 - 1)
            gts.append((torch.from_numpy(np.asarray(gt).astype(np.float32) / 255.)[None]) * 2 - 1)
        torch.stack(rgbs), torch.stack(gts)
        ms.append((time.perf_counter() - t0) * 1e3)
    return median3(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=4, help="training steps timed (after --warmup steps)")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from adm_amd import hip
    from adm_amd.ddm.pair_data import DUTSBatchStream, pair_batch
    from train_uncond_dpm import Cfg, build_model
    hip.lib()
    dev = torch.device("cuda", 0)
    cfg = yaml.load(open(os.path.join(ROOT, "configs/saliency/duts_cond_ddm_const_ldm.yaml")), Loader=yaml.SafeLoader)
    cfg["data"].update(class_name="synthetic", synthetic_of="ddm.data.DUTSDataset", batch_size=args.batch)
    cfg = Cfg(cfg)
    size = (int(cfg.data.image_size[0]), int(cfg.data.image_size[1]))
    stream = DUTSBatchStream(cfg.data, args.batch, size, dev, seed=1)
    idx, flip = stream.draw()
    res = {"what": "saliency training batches (adm_pair_resize_batch) on one MI355X; ms = median (min, max)", "batch": args.batch,
           "size": list(size), "reps": args.reps, "pool_pairs": stream.pool.n, "pool_bytes": stream.pool.nbytes,
           "source_sizes": sorted({(int(h), int(w)) for h, w in stream.pool.hw_host[0]}),
           "resize_tables": len(stream.pool.tables["keys"])}
    res["batch_kernel_ms"] = timed(lambda: pair_batch(stream.pool, idx, flip), args.warmup, args.reps)
    res["stream_ms_per_batch_with_device_draws"] = timed(lambda: next(stream), args.warmup, args.reps)
    res["output_MB_per_batch"] = round(args.batch * 4 * 4 * size[0] * size[1] / 1e6, 2)
    pairs, flips = host_pairs(stream.pool, idx.tolist()), flip.tolist()
    res["host_numpy_ms_per_batch_one_process"] = host_numpy_ms(pairs, flips, size, max(3, args.reps // 4))
    res["host_pil_ms_per_batch_one_process"] = host_pil_ms(pairs, flips, size, max(3, args.reps // 4))
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
                             "model": "ddm_const.LatentDiffusion, one-channel KL-f4 first stage at 384x384, unet.cond_unet.Unet dim 128 x "
                                      "(1,2,4,4), Swin-B encoder trained"}
        res["batches_share_of_step_percent"] = round(100.0 * accum * res["stream_ms_per_batch_with_device_draws"][0] / res["train_step_ms"][0], 3)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
