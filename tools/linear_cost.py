#!/usr/bin/env python3
"""Cost of the linear-drift recipe (ddm.ddm_linear) against the const recipe, full-size CIFAR-10 models (bench.py's model and step,
bs=128, fp32), in ONE process.

  python tools/linear_cost.py --mode time --out profiles/linear_cost.json
      two models (identical UNets apart from the head's outputs), each with its own optimiser; blocks of --steps training steps
      alternate between the const recipe and the linear recipe, --rounds times, device-synchronised after warm-up; then one
      sample(--batch) of each (const: 10 network evaluations, deterministic; linear: 11, stochastic Euler).  Reports ms/step of
      both, their difference, the spread across rounds and sampled images/s.  The yardstick is the const step of the same call.
  rocprofv3 --kernel-trace --stats ... -- python tools/linear_cost.py --mode profile --steps 5
      the linear step alone, for a kernel trace (a run of its own)

Both recipes run with perceptual_weight = 0 (no LPIPS weights ship); the linear loss_vlb then is its MAE part, which is inside the
fused loss launch.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_linear(dev, const_dpm):
    """bench.build_model's CIFAR-10 model with the K | C head and the linear wrapper; every shared parameter copied from the const
    model, so both do the same UNet work on the same values."""
    from adm_amd.ddm.ddm_linear import DDPM
    from adm_amd.unet.uncond_unet import EDMPrecond
    kw = dict(model_channels=192, channel_mult=[1, 2, 2, 2], channel_mult_emb=4, num_blocks=3, attn_resolutions=[16, 8],
              dropout=0.1, label_dropout=0, augment_dim=9)
    torch.manual_seed(1234)
    unet = EDMPrecond(img_resolution=32, img_channels=3, sigma_data=1.0, model_type="DhariwalUNet", out_mul=2, precondition=False, **kw)
    src = const_dpm.model.state_dict()
    with torch.no_grad():
        for k, v in unet.state_dict().items():
            if tuple(src[k].shape) == tuple(v.shape):
                v.copy_(src[k])
            else:           # the head: the const head's rows for K, the same again for C
                v.copy_(torch.cat([src[k].cpu(), src[k].cpu()], dim=0))
    mcfg = dict(eps=1e-4, sigma_max=1, sigma_min=0.01, weighting_loss=True, use_augment=False, ldm=False)
    dpm = DDPM(model=unet, image_size=[32, 32], sampling_timesteps=10, loss_type="l2", start_dist="normal", perceptual_weight=0.0,
               use_l1=False, cfg=mcfg)
    return dpm.to(dev)


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
    models = {"const": bench.build_model(dev, False, "cifar", False)}
    models["linear"] = build_linear(dev, models["const"])
    gen = torch.Generator(device=dev).manual_seed(100)
    batches = [{"image": torch.rand(args.batch, 3, 32, 32, device=dev, generator=gen) * 2 - 1} for _ in range(2)]
    state = {}
    for name, dpm in models.items():
        dpm.train()
        flat = FlatParams(dpm)
        state[name] = (dpm, flat, BucketedGradReducer(flat), FusedAdamWEMA(flat, lr=1e-4, weight_decay=1e-4, max_norm=1.0, ema=True))

    def train_step(name, it):
        dpm, flat, reducer, opt = state[name]
        flat.zero_grad()
        loss, log = dpm.training_step(batches[it & 1])
        loss.backward()
        reducer.finish()
        opt.step(lr=1e-4 * lr_lambda(400000 + it, 1e-4, 5e-6, 800000), grad_scale=1.0,
                 ema_decay=ema_decay_at(400000 + it) if (it % 8 == 0) else None)
        return loss

    def block(name, n, it0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            loss = train_step(name, it0 + i)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / n
        assert torch.isfinite(loss).all(), (name, float(loss))
        return ms

    it = 0
    names = ("linear",) if args.mode == "profile" else ("const", "linear")
    for name in names:
        block(name, args.warmup, it)
        it += args.warmup
    if args.mode == "profile":
        ms = block("linear", args.steps, it)
        print(f"profile: {args.warmup} + {args.steps} steps of the linear recipe, {ms:.2f} ms/step under the tracer")
        return
    ms = {"const": [], "linear": []}
    for r in range(args.rounds):
        for name in names:
            ms[name].append(round(block(name, args.steps, it), 3))
            it += args.steps

    def sample_rate(name):
        dpm = state[name][0].eval()
        dpm.sample(batch_size=args.batch)                # warm-up (packs nothing new, fills the allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = dpm.sample(batch_size=args.batch)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert tuple(img.shape) == (args.batch, 3, 32, 32) and torch.isfinite(img).all()
        return round(args.batch / dt, 1)

    rates = {name: sample_rate(name) for name in names}
    mean = lambda v: sum(v) / len(v)
    diff = mean(ms["linear"]) - mean(ms["const"])
    spread = {k: round(max(v) - min(v), 3) for k, v in ms.items()}
    head = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    res = {"what": "full-size CIFAR-10 training step (216M-parameter UNet, fp32, optimiser and EMA included) and one sample(batch), "
                   "const recipe against linear recipe in one process, one MI355X",
           "batch": args.batch, "steps_per_block": args.steps, "rounds": args.rounds,
           "ms_per_step_const": ms["const"], "ms_per_step_linear": ms["linear"],
           "mean_const": round(mean(ms["const"]), 3), "mean_linear": round(mean(ms["linear"]), 3),
           "linear_minus_const_ms_per_step": round(diff, 3), "linear_minus_const_percent": round(100.0 * diff / mean(ms["const"]), 2),
           "spread_const_ms": spread["const"], "spread_linear_ms": spread["linear"],
           "difference_exceeds_spread": bool(abs(diff) > max(spread.values())),
           "sampled_images_per_s_const": rates["const"], "sampled_images_per_s_linear": rates["linear"],
           "network_evaluations_per_sample_call": {"const": 10, "linear": 11},
           "git_head": head}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
