#!/usr/bin/env python3
"""Cost of one training step of the KL autoencoder at the recipe's real size (configs/celebahq/celeb_ae_kl_256x256_d4.yaml:
B = 8, 256x256, ch = 128), fp32, one MI355X, optimiser steps (torch.optim.AdamW) included.

  python tools/ae_train_cost.py --mode time --out profiles/ae_train_cost.json
      device events around each micro-step: blocks of --steps autoencoder micro-steps, discriminator micro-steps and forward-only
      ae(x) passes (the anchor the step is read against) alternate --rounds times in one call, after a warm-up of every shape
  rocprofv3 --kernel-trace --stats ... -- python tools/ae_train_cost.py --mode profile --steps 3
      both micro-steps for a kernel trace (a run of its own)

The LPIPS weights are synthetic (hash-filled VGG16, He-scaled: the real ones do not ship and are never fetched; the cost does not
depend on their values); the lin weights are tests/golden/lpips_lin.pt.  global_step is past disc_start, so the discriminator
contributes to both micro-steps.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["time", "profile"], default="time")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--ch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from adm_amd import hip
    from adm_amd.ddm.encoder_decoder import AutoencoderKL
    from lpips_cost import synthetic_lpips
    hip.lib()
    dev = torch.device("cuda", 0)
    dd = dict(double_z=True, z_channels=3, resolution=[args.size, args.size], in_channels=3, out_ch=3, ch=args.ch, ch_mult=[1, 2, 4],
              num_res_blocks=2, attn_resolutions=[], dropout=0.0)
    torch.manual_seed(0)
    ae = AutoencoderKL(dd, dict(disc_start=0, kl_weight=1e-6, disc_weight=0.5), 3).to(dev)
    ae.enable_training(lpips=synthetic_lpips()).train()
    ae_params = (list(ae.encoder.parameters()) + list(ae.decoder.parameters()) + list(ae.quant_conv.parameters())
                 + list(ae.post_quant_conv.parameters()))
    opts = [torch.optim.AdamW(ae_params, lr=5e-6), torch.optim.AdamW(ae.loss.discriminator.parameters(), lr=5e-6)]
    gen = torch.Generator(device=dev).manual_seed(100)
    batches = [torch.rand(args.batch, 3, args.size, args.size, device=dev, generator=gen) * 2 - 1 for _ in range(2)]

    def micro(idx, it):
        for o in opts[idx:]:
            o.zero_grad(set_to_none=True)
        _, log = ae.training_step(batches[it & 1], idx, 10 + it, loss_scale=0.5)
        opts[idx].step()
        return log

    def forward_only(_, it):
        ae.eval()
        with torch.no_grad():
            ae(batches[it & 1])
        ae.train()

    def block(fn, idx, n, it0):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for i in range(n):
            fn(idx, it0 + i)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n

    kinds = (("ae_micro_step", micro, 0), ("disc_micro_step", micro, 1), ("forward_only", forward_only, None))
    it = 0
    for _, fn, idx in kinds:
        block(fn, idx, args.warmup, it)
        it += args.warmup
    if args.mode == "profile":
        for _, fn, idx in kinds[:2]:
            block(fn, idx, args.steps, it)
            it += args.steps
        return
    ms = {k: [] for k, _, _ in kinds}
    for _ in range(args.rounds):
        for k, fn, idx in kinds:
            ms[k].append(round(block(fn, idx, args.steps, it), 3))
            it += args.steps
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    log = micro(0, it)
    res = {"what": f"KL autoencoder training at B={args.batch}, {args.size}x{args.size}, ch={args.ch}, fp32, one MI355X; device events, "
                   f"AdamW steps included; {args.rounds} rounds of {args.steps} timed steps per kind, alternated in one call",
           "batch": args.batch, "steps_per_block": args.steps, "rounds": args.rounds,
           "ms_per_step": ms, "mean_ms": {k: round(v, 3) for k, v in mean.items()},
           "spread_ms": {k: round(max(v) - min(v), 3) for k, v in ms.items()},
           "images_per_s_for_the_pair": round(args.batch / ((mean["ae_micro_step"] + mean["disc_micro_step"]) * 1e-3), 2),
           "pair_over_forward_only": round((mean["ae_micro_step"] + mean["disc_micro_step"]) / mean["forward_only"], 2),
           "weights": "synthetic VGG16 (hash-filled, He-scaled) + the real lin weights; random autoencoder / discriminator init",
           "last_log": {k: float(v) for k, v in log.items()}}
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
