#!/usr/bin/env python3
"""Cost of the LPIPS term on the full-size CIFAR-10 training step (bench.py's model and step, bs=128, fp32).

  python tools/lpips_cost.py --mode time --out profiles/lpips_cost.json
      one model, one optimiser; blocks of --steps steps alternate between perceptual_weight = 0 and 1 (the weight gates the
      term, so flipping it is the whole difference), --rounds times; reports ms/step of both and the difference
  rocprofv3 --kernel-trace --stats ... -- python tools/lpips_cost.py --mode profile --steps 5
      the step with the term on, for a kernel trace (a run of its own)

The VGG16 weights are synthetic (hash-filled, He-scaled: the real ones do not ship and are never fetched; the cost does not
depend on their values); the lin weights are tests/golden/lpips_lin.pt.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_lpips():
    from adm_amd.ddm.lpips import LPIPS, SLICES
    from oracle import fill
    vgg = {}
    for sl in SLICES:
        for i, ci, co in sl:
            vgg[f"features.{i}.weight"] = fill.hash_tensor((co, ci, 3, 3), f"vgg.features.{i}.weight", (6.0 / (ci * 9)) ** 0.5)
            vgg[f"features.{i}.bias"] = 0.05 + fill.hash_tensor((co,), f"vgg.features.{i}.bias", 0.03)
    lin = torch.load(os.path.join(ROOT, "tests", "golden", "lpips_lin.pt"), map_location="cpu", weights_only=True)
    return LPIPS.from_vgg16(vgg, lin)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["time", "profile"], default="time")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import bench
    from adm_amd import hip
    from adm_amd.optim import BucketedGradReducer, FlatParams, FusedAdamWEMA, ema_decay_at, lr_lambda
    hip.lib()
    dev = torch.device("cuda", 0)
    dpm = bench.build_model(dev, False, "cifar", False)
    dpm.set_perceptual_loss(synthetic_lpips())
    dpm.train()
    flat = FlatParams(dpm)
    reducer = BucketedGradReducer(flat)
    opt = FusedAdamWEMA(flat, lr=1e-4, weight_decay=1e-4, max_norm=1.0, ema=True)
    gen = torch.Generator(device=dev).manual_seed(100)
    batches = [{"image": torch.rand(args.batch, 3, 32, 32, device=dev, generator=gen) * 2 - 1} for _ in range(2)]

    def train_step(it):
        flat.zero_grad()
        loss, log = dpm.training_step(batches[it & 1])
        loss.backward()
        reducer.finish()
        opt.step(lr=1e-4 * lr_lambda(400000 + it, 1e-4, 5e-6, 800000), grad_scale=1.0,
                 ema_decay=ema_decay_at(400000 + it) if (it % 8 == 0) else None)
        return log

    def block(weight, n, it0):
        dpm.perceptual_weight = weight
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            log = train_step(it0 + i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, float(log["train/loss_vlb"])

    it = 0
    for w in (0.0, 1.0):
        block(w, args.warmup, it)
        it += args.warmup
    if args.mode == "profile":
        ms, vlb = block(1.0, args.steps, it)
        print(f"profile: {args.steps} steps with the LPIPS term, {ms:.2f} ms/step under the tracer, train/loss_vlb {vlb:.3e}")
        return
    off, on = [], []
    for r in range(args.rounds):
        for w, acc in ((0.0, off), (1.0, on)):
            ms, vlb = block(w, args.steps, it)
            it += args.steps
            acc.append(round(ms, 3))
            assert (vlb > 0) == (w > 0), (w, vlb)
    mean = lambda v: sum(v) / len(v)
    res = {"what": "full-size CIFAR-10 training step (216M-parameter UNet, fp32, optimiser and EMA included), one MI355X",
           "batch": args.batch, "steps_per_block": args.steps, "rounds": args.rounds,
           "ms_per_step_without_lpips": off, "ms_per_step_with_lpips": on,
           "mean_without": round(mean(off), 3), "mean_with": round(mean(on), 3),
           "added_ms_per_step": round(mean(on) - mean(off), 3),
           "added_percent": round(100.0 * (mean(on) - mean(off)) / mean(off), 2),
           "spread_without_ms": round(max(off) - min(off), 3), "spread_with_ms": round(max(on) - min(on), 3),
           "weights": "synthetic VGG16 (hash-filled, He-scaled) + the real lin weights"}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
