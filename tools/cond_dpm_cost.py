#!/usr/bin/env python3
"""Cost of the pixel-space saliency recipe (configs/saliency/duts_cond_ddm_const_dpm.yaml) at its own shape -- B = 12, 1x128x128,
2 micro-batches per step, Swin-B trained along -- in ONE process on one MI355X.

  python tools/cond_dpm_cost.py --out profiles/cond_dpm_cost.json

1. The two new kernels against the same work composed from what existed, device events around --iters calls, the two forms
   alternating, --rounds times (microsecond-scale launches: the yardstick is existing code of the same call, not a bar):
     loss        ops.ddm_loss_l1 + backward         against  ops.ddm_loss + torch ops for the two mean-|.| terms + backward
     lpips input ops.lpips_input on [B,1,H,W]       against  expand to three channels + the three-channel kernel (its backward
                 + backward, schedule 0 ('const')            sums the channels with a torch reduction)
2. The whole training step (2 micro-batches of 12 synthetic DUTS pairs, optimiser and EMA included, LPIPS active on synthetic VGG16
   weights) and the share of it the new kernels take (per micro-batch: one loss launch, the prediction's input forward and
   backward, the target's input forward -- from the timings of 1).
3. sample() of 12 photos with the encoder run once per call (sample(cond=photo)) and once per step (sample_fn_d given the photo).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def event_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(forms, iters, rounds, warmup=20):
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            out[k].append(round(event_us(fn, iters), 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from adm_amd import hip, ops
    from adm_amd.ddm.pair_data import DUTSBatchStream
    from adm_amd.optim import BucketedGradReducer, FlatParams, FusedAdamWEMA, ema_decay_at, lr_lambda_cond
    from lpips_cost import synthetic_lpips
    from train_uncond_dpm import Cfg, build_model
    hip.lib()
    dev = torch.device("cuda", 0)
    with open(os.path.join(ROOT, "configs", "saliency", "duts_cond_ddm_const_dpm.yaml")) as f:
        cfg = Cfg(yaml.load(f, Loader=yaml.SafeLoader))
    B, (H, W) = int(cfg.data.batch_size), cfg.model.image_size
    gen = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)

    # ---- 1. the kernels against their composed forms
    c, e, x0, noise = (rnd(B, 1, H, W) for _ in range(4))
    t = torch.rand(B, device=dev, generator=gen) * 0.98 + 0.01
    w = torch.stack([(t ** 2 - t + 1) / t, (t ** 2 - t + 1) / (1 - t + 1e-4)], dim=1).contiguous()
    cg, eg = c.clone().requires_grad_(True), e.clone().requires_grad_(True)

    def loss_new():
        cg.grad = eg.grad = None
        ops.ddm_loss_l1(cg, eg, x0, noise, w)[0].backward()

    def loss_composed():
        cg.grad = eg.grad = None
        sse = ops.ddm_loss(cg, eg, x0, noise, w)[0]
        l1 = (w[:, 0] * (cg + x0).abs().mean([1, 2, 3]) + w[:, 1] * (eg - noise).abs().mean([1, 2, 3])).sum() / B
        ((sse + l1) / 2).backward()

    loss_new(); g_new = (cg.grad.clone(), eg.grad.clone())
    loss_composed()
    assert torch.allclose(cg.grad, g_new[0], rtol=1e-4, atol=1e-7) and torch.allclose(eg.grad, g_new[1], rtol=1e-4, atol=1e-7)
    shift = torch.tensor([-.030, -.088, -.188], device=dev)
    scale = torch.tensor([.458, .448, .450], device=dev)
    gy = rnd(B, H, W, 32)

    def input_new():
        cg.grad = None
        ops.lpips_input(cg, None, None, None, shift, scale, 0).backward(gy)

    def input_composed():
        cg.grad = None
        ops.lpips_input(cg.expand(-1, 3, -1, -1), None, None, None, shift, scale, 0).backward(gy)

    input_new(); g_in = cg.grad.clone()
    input_composed()
    assert torch.allclose(cg.grad, g_in, rtol=1e-5, atol=1e-6)
    with torch.no_grad():
        assert torch.equal(ops.lpips_input(c, None, None, None, shift, scale, 0),
                           ops.lpips_input(c.expand(-1, 3, -1, -1), None, None, None, shift, scale, 0))
    target_new = lambda: ops.lpips_input(x0, None, None, None, shift, scale, -1)
    target_composed = lambda: ops.lpips_input(x0.expand(-1, 3, -1, -1), None, None, None, shift, scale, -1)
    us = alternate({"loss_new": loss_new, "loss_composed": loss_composed, "input_fwd_bwd_new": input_new,
                    "input_fwd_bwd_composed": input_composed, "input_fwd_new": target_new, "input_fwd_composed": target_composed},
                   args.iters, args.rounds)
    mean = lambda v: sum(v) / len(v)
    kernels = {k: {"us_per_call": v, "mean_us": round(mean(v), 2), "spread_us": round(max(v) - min(v), 2)} for k, v in us.items()}
    ratios = {k: round(mean(us[k + "_new"]) / mean(us[k + "_composed"]), 3) for k in ("loss", "input_fwd_bwd", "input_fwd")}

    # ---- 2. the training step
    torch.manual_seed(1234)
    dpm = build_model(cfg.model).to(dev)
    dpm.set_perceptual_loss(synthetic_lpips())
    dpm.train()
    flat = FlatParams(dpm)
    reducer = BucketedGradReducer(flat)
    opt = FusedAdamWEMA(flat, lr=5e-5, weight_decay=1e-2, max_norm=1.0, ema=True)
    stream = DUTSBatchStream(cfg.data, B, (H, W), dev, seed=1000)
    accum = int(cfg.trainer.gradient_accumulate_every)

    def train_step(it):
        flat.zero_grad()
        for ga in range(accum):
            loss, log = dpm.training_step(next(stream))
            (loss / accum).backward()
        reducer.finish()
        opt.step(lr=5e-5 * lr_lambda_cond(it, 5e-5, 5e-6, 400000), grad_scale=1.0, ema_decay=ema_decay_at(30000 + it) if it % 4 == 0 else None)
        return loss, log

    for it in range(args.warmup):
        train_step(it)
    step_ms = []
    for r in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            loss, log = train_step(args.warmup + r * args.steps + i)
        torch.cuda.synchronize()
        step_ms.append(round((time.perf_counter() - t0) * 1e3 / args.steps, 2))
        assert torch.isfinite(loss).all() and float(log["train/loss_vlb"]) > 0
    new_us = accum * (mean(us["loss_new"]) + mean(us["input_fwd_bwd_new"]) + mean(us["input_fwd_new"]))

    # ---- 3. sample(): the encoder once per call against once per step
    dpm.eval()
    photo = next(stream)["cond"]
    n_steps = int(cfg.model.sampling_timesteps)

    def sample_ms(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = fn()
        torch.cuda.synchronize()
        assert tuple(img.shape) == (B, 1, H, W) and torch.isfinite(img).all()
        return round((time.perf_counter() - t0) * 1e3, 2)

    forms = {"encoder_once": lambda: dpm.sample(cond=photo), "encoder_per_step": lambda: dpm.sample_fn_d((B, 1, H, W), cond=photo)}
    sample = {k: [] for k in forms}
    for r in range(args.rounds):
        for k, fn in forms.items():
            sample[k].append(sample_ms(fn))

    head = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    res = {"what": f"pixel-space saliency recipe, B = {B}, 1x{H}x{W}, {accum} micro-batches per step, Swin-B trained along, fp32, one MI355X",
           "iters_per_timing": args.iters, "rounds": args.rounds, "kernels": kernels, "new_over_composed": ratios,
           "train_step_ms": step_ms, "train_step_mean_ms": round(mean(step_ms), 2), "train_step_spread_ms": round(max(step_ms) - min(step_ms), 2),
           "new_kernels_us_per_step": round(new_us, 1), "new_kernels_share_of_step_percent": round(100.0 * new_us / (mean(step_ms) * 1e3), 4),
           "lpips_weights": "synthetic VGG16 (hash-filled, He-scaled) + the real lin weights",
           "sample_ms": sample, "sample_mean_ms": {k: round(mean(v), 2) for k, v in sample.items()},
           "sample_network_evaluations": n_steps, "sample_encoder_runs": {"encoder_once": 1, "encoder_per_step": n_steps},
           "git_head": head}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
