#!/usr/bin/env python3
"""Cost of the saliency score on one MI355X, next to the sampled image it scores.

  python tools/saliency_metrics_cost.py --out profiles/saliency_metrics_cost.json

Figures (ms = median (min, max)):
  * one ``adm_saliency_tables`` launch at 384x384 for B = 1 and B = 8, on uniform-random bytes and on a SATURATED pair (a 0/255 map
    with a 0/255 prediction: what real maps look like, and the worst case for a histogram's atomics), as bytes and as a float32
    prediction.  Device events around --launches back-to-back launches, divided; medians over --reps windows after warm-up, the two
    inputs alternating inside one loop so that they share whatever else the machine is doing.  The launches are the raw C-ABI call on
    buffers made once; ``enqueue_ms`` is the host's time per call in the same windows, and ``single_launch_ms`` one launch between two
    events (which adds the events' own cost): the kernel's time lies below both;
  * the host half (``metrics_from_tables``) per image, and on this host's CPU np.bincount for the same tables and the per-pixel
    restatement (tests/saliency_ref.py) for the whole score of one image;
  * one sampled image of configs/saliency/duts_cond_ddm_const_ldm_sample.yaml (384x384, one window, 10 steps, random weights) and the
    launch's share of it.
The point of the kernel is the project's rule that nothing on a metric path falls back to the CPU or to eager PyTorch, not speed: the
share says how little there was to win."""
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


def median3(ms, digits=4):
    return [round(statistics.median(ms), digits), round(min(ms), digits), round(max(ms), digits)]


def window_ms(fn, launches):
    """(device ms, host enqueue ms) per launch of `launches` back-to-back calls: where the two are equal the host's enqueue rate is what
    was measured, and the kernel takes less."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(launches):
        fn()
    t1 = time.perf_counter()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches, (t1 - t0) * 1e3 / launches


def host_ms(fn, reps):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return median3(ms, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--launches", type=int, default=50, help="back-to-back launches per timed window")
    ap.add_argument("--skip-sample", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import saliency_ref as R
    from adm_amd import hip
    from adm_amd.metrics.saliency import metrics_from_tables, saliency_tables
    from train_uncond_dpm import Cfg, build_model
    hip.lib()
    dev = torch.device("cuda", 0)
    H = W = args.size
    res = {"what": "saliency score (adm_saliency_tables + host half) on one MI355X; ms = median (min, max) per launch",
           "size": [H, W], "reps": args.reps, "launches_per_window": args.launches}
    gen = torch.Generator(device=dev).manual_seed(5)
    for B in (1, 8):
        uni = [torch.randint(0, 256, (B, H, W), device=dev, dtype=torch.uint8, generator=gen) for _ in range(2)]
        sat = [((torch.rand(B, H, W, device=dev, generator=gen) < q) * 255).to(torch.uint8) for q in (0.4, 0.3)]
        # (a block-shaped saturated pair as well: long runs, as in a real map)
        blk = [torch.zeros(B, H, W, device=dev, dtype=torch.uint8) for _ in range(2)]
        blk[0][:, H // 4:H // 2, W // 3:W // 3 * 2] = 255
        blk[1][:, H // 4 + 9:H // 2 + 5, W // 3 - 7:W // 3 * 2] = 255
        forms = {"uniform_u8": uni, "saturated_noise_u8": sat, "saturated_blocks_u8": blk,
                 "uniform_f32": [(uni[0].float() / 255).contiguous(), uni[1]], "saturated_blocks_f32": [(blk[0].float() / 255).contiguous(), blk[1]]}
        for name, (p, m) in forms.items():          # what is timed is what is right
            tables, head = saliency_tables(p, m)
            q = (p.float() * 255).round().to(torch.uint8) if p.dtype == torch.float32 else p
            want = [R.tables_ref(a, b) for a, b in zip(q.cpu().numpy(), m.cpu().numpy())]
            assert np.array_equal(tables.cpu().numpy(), np.stack([t for t, _ in want])), name
            assert np.array_equal(head.cpu().numpy(), np.stack([h for _, h in want])), name
        tables, head = torch.empty(B, 4, 2, 256, device=dev, dtype=torch.int64), torch.empty(B, 5, device=dev, dtype=torch.int64)
        raw = lambda p, m: hip.call("adm_saliency_tables", hip.ptr(p), int(p.dtype == torch.float32), hip.ptr(m), hip.ptr(tables),
                                    hip.ptr(head), B, H, W)
        ms, enq, single = {name: [] for name in forms}, {name: [] for name in forms}, {name: [] for name in forms}
        for it in range(args.warmup + args.reps):
            for name, (p, m) in forms.items():
                v, e = window_ms(lambda: raw(p, m), args.launches)
                one, _ = window_ms(lambda: raw(p, m), 1)
                if it >= args.warmup:
                    ms[name].append(v), enq[name].append(e), single[name].append(one)
        for name in forms:
            res[f"launch_ms_B{B}_{name}"] = median3(ms[name])
            res[f"enqueue_ms_B{B}_{name}"] = median3(enq[name])
            res[f"single_launch_ms_B{B}_{name}"] = median3(single[name])
        res[f"saturated_over_uniform_B{B}"] = round(max(res[f"launch_ms_B{B}_saturated_noise_u8"][0], res[f"launch_ms_B{B}_saturated_blocks_u8"][0])
                                                    / res[f"launch_ms_B{B}_uniform_u8"][0], 3)
        if B == 1:
            p, m = uni[0][0].cpu().numpy(), uni[1][0].cpu().numpy()
            tables, head = R.tables_ref(p, m)
            res["host_half_ms_per_image"] = host_ms(lambda: metrics_from_tables(tables[None], head[None], (H, W)), 5)
            res["host_bincount_tables_ms_per_image"] = host_ms(lambda: R.tables_ref(p, m), 5)
            res["host_per_pixel_restatement_ms_per_image"] = host_ms(lambda: R.image_ref(p, m), 3)
    res["host_cpus_visible"] = os.cpu_count()
    if not args.skip_sample:
        import sample_cond_ldm as S
        scfg = Cfg(yaml.load(open(os.path.join(ROOT, "configs", "saliency", "duts_cond_ddm_const_ldm_sample.yaml")), Loader=yaml.SafeLoader))
        torch.manual_seed(8)
        ldm = build_model(scfg.model).to(dev).eval()
        size = tuple(scfg.data.image_size)
        crop, stride = tuple(scfg.sampler.crop_size), tuple(scfg.sampler.stride)
        batch = {"cond": torch.rand(1, 3, *size, device=dev) * 2 - 1}

        def image():
            with torch.no_grad():
                return S.predict_slide(ldm, scfg.sampler, batch, crop, stride)

        for _ in range(2):
            pred = image()
        torch.cuda.synchronize()
        ms = []
        for _ in range(4):
            t0 = time.perf_counter()
            pred = image()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        assert tuple(pred.shape) == (1, 1) + size and bool(torch.isfinite(pred).all())
        res["sampled_image_ms"] = median3(ms, 1)
        res["sampled_image"] = {"size": list(size), "windows": 1, "sampling_timesteps": int(scfg.model.sampling_timesteps), "images_timed": len(ms)}
        worst = max(res[f"launch_ms_B1_{n}"][0] for n in ("uniform_f32", "saturated_blocks_f32"))
        res["launch_share_of_sampled_image_percent"] = round(100.0 * worst / res["sampled_image_ms"][0], 4)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
