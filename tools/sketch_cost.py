#!/usr/bin/env python3
"""Cost of the sketch-to-image recipe (configs/sketch2img/sketchcoco_cond_ddm_const_ldm.yaml) at its own shape -- B = 16, 1x256x256
sketches, 3x256x256 photos, 2 micro-batches per step, the one-channel Swin-B trained along -- in ONE process on one MI355X.

  python tools/sketch_cost.py --out profiles/sketch_cost.json

1. The fused stem (ops_swin.patch_embed_ln: adm_patch_embed_ln_fwd / _bwd) against the same work composed from what existed before
   it -- ops.nchw_to_nhwc padding the sketch to 32 channels, ops_cond.conv2d_generic(stride 4) as a K = 512 GEMM, ops_swin.layer_norm
   -- forward alone and forward + backward (parameter gradients), at E = 128.  Device events around --iters calls, the two forms
   alternating, --rounds times.  The composed form is the yardstick: the fused kernel should not be slower.  The forward's bytes
   (x read once, y written once) over its time are reported as an achieved rate, named for what it is.
2. The whole training step (2 micro-batches of 16 synthetic pairs, optimiser and EMA included) and the share of it the stem takes
   (per micro-batch one forward and one backward, from the timings of 1).
3. sample() of 16 sketches (the encoder runs once per call).
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

from cond_dpm_cost import alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from adm_amd import hip, ops
    from adm_amd import ops_cond as oc
    from adm_amd import ops_swin as osw
    from adm_amd.ddm.pair_data import SketchBatchStream
    from adm_amd.optim import BucketedGradReducer, FlatParams, FusedAdamWEMA, ema_decay_at, lr_lambda_cond
    from train_uncond_dpm import Cfg, build_model
    hip.lib()
    dev = torch.device("cuda", 0)
    with open(os.path.join(ROOT, "configs", "sketch2img", "sketchcoco_cond_ddm_const_ldm.yaml")) as f:
        cfg = Cfg(yaml.load(f, Loader=yaml.SafeLoader))
    B, (H, W), E = int(cfg.data.batch_size), cfg.model.image_size, 128
    gen = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)

    # ---- 1. the fused stem against its composed form
    x = rnd(B, 1, H, W)
    dy = rnd(B, H // 4, W // 4, E)
    params = [(rnd(E, 1, 4, 4) * 0.25), rnd(E) * 0.1, 1.0 + rnd(E) * 0.1, rnd(E) * 0.1]
    pg = [p.clone().requires_grad_(True) for p in params]

    def fused(ps):
        return osw.patch_embed_ln(x, *ps, 1e-5)

    def composed(ps):
        h = oc.conv2d_generic(ops.nchw_to_nhwc(x, None, 32), ps[0], ps[1], stride=4, pad=0)
        return osw.layer_norm(h, ps[2], ps[3], 1e-5)

    def fwd_bwd(form):
        def run():
            for p in pg:
                p.grad = None
            form(pg).backward(dy)
        return run

    with torch.no_grad():
        ya, yb = fused(params), composed(params)
    assert torch.allclose(ya, yb, rtol=1e-4, atol=1e-5), float((ya - yb).abs().max())
    fwd_bwd(fused)(); g_new = [p.grad.clone() for p in pg]
    fwd_bwd(composed)()
    for a, p in zip(g_new, pg):
        assert torch.allclose(a, p.grad, rtol=1e-3, atol=1e-3 * float(a.abs().max())), float((a - p.grad).abs().max())
    nograd = lambda form: (lambda: form(params))
    with torch.no_grad():
        us_f = alternate({"fwd_new": nograd(fused), "fwd_composed": nograd(composed)}, args.iters, args.rounds)
    us_b = alternate({"fwd_bwd_new": fwd_bwd(fused), "fwd_bwd_composed": fwd_bwd(composed)}, args.iters, args.rounds)
    us = {**us_f, **us_b}
    mean = lambda v: sum(v) / len(v)
    kernels = {k: {"us_per_call": v, "mean_us": round(mean(v), 2), "spread_us": round(max(v) - min(v), 2)} for k, v in us.items()}
    ratios = {k: round(mean(us[k + "_new"]) / mean(us[k + "_composed"]), 3) for k in ("fwd", "fwd_bwd")}
    fwd_bytes = 4 * (x.numel() + ya.numel())
    del ya, yb

    # ---- 2. the training step
    torch.manual_seed(1234)
    ldm = build_model(cfg.model).to(dev).train()
    flat = FlatParams(ldm)
    reducer = BucketedGradReducer(flat)
    opt = FusedAdamWEMA(flat, lr=5e-5, weight_decay=1e-2, max_norm=1.0, ema=True)
    stream = SketchBatchStream(cfg.data, B, (H, W), dev, seed=1000)
    accum = int(cfg.trainer.gradient_accumulate_every)
    first = next(stream)
    ldm.on_train_batch_start(first)

    def train_step(it):
        flat.zero_grad()
        for ga in range(accum):
            loss, log = ldm.training_step(next(stream))
            (loss / accum).backward()
        reducer.finish()
        opt.step(lr=5e-5 * lr_lambda_cond(it, 5e-5, 5e-6, 300000), grad_scale=1.0, ema_decay=ema_decay_at(30000 + it) if it % 8 == 0 else None)
        return loss

    for it in range(args.warmup):
        train_step(it)
    step_ms = []
    for r in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            loss = train_step(args.warmup + r * args.steps + i)
        torch.cuda.synchronize()
        step_ms.append(round((time.perf_counter() - t0) * 1e3 / args.steps, 2))
        assert torch.isfinite(loss).all()
    stem_us = accum * mean(us["fwd_bwd_new"])
    stem_composed_us = accum * mean(us["fwd_bwd_composed"])

    # ---- 3. sample() of B sketches
    ldm.eval()
    sketch = first["cond"]

    def sample_ms():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            img = ldm.sample(cond=sketch)
        torch.cuda.synchronize()
        assert tuple(img.shape) == (B, 3, H, W) and torch.isfinite(img).all()
        return round((time.perf_counter() - t0) * 1e3, 2)

    sample_ms()
    sample = [sample_ms() for _ in range(args.rounds)]

    head = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    res = {"what": f"sketch-to-image recipe, B = {B}, sketch 1x{H}x{W}, photo 3x{H}x{W}, {accum} micro-batches per step, one-channel Swin-B "
                   "trained along, fp32, one MI355X",
           "stem_shape": {"B": B, "H": H, "W": W, "E": E}, "iters_per_timing": args.iters, "rounds": args.rounds,
           "kernels": kernels, "new_over_composed": ratios,
           "fwd_bytes_read_plus_written": fwd_bytes,
           "fwd_new_achieved_GBps_bytes_over_event_time": round(fwd_bytes / (mean(us["fwd_new"]) * 1e-6) / 1e9, 1),
           "train_step_ms": step_ms, "train_step_mean_ms": round(mean(step_ms), 2), "train_step_spread_ms": round(max(step_ms) - min(step_ms), 2),
           "stem_us_per_step": round(stem_us, 1), "stem_share_of_step_percent": round(100.0 * stem_us / (mean(step_ms) * 1e3), 4),
           "composed_stem_us_per_step": round(stem_composed_us, 1),
           "sample_ms": sample, "sample_mean_ms": round(mean(sample), 2), "sample_network_evaluations": int(cfg.model.sampling_timesteps),
           "git_head": head}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
