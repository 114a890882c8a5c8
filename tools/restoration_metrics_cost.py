#!/usr/bin/env python3
"""Cost of the restoration score on one MI355X, next to the sampled image it scores.

  python tools/restoration_metrics_cost.py --out profiles/restoration_metrics_cost.json

Figures (ms = median (min, max)):
  * one ``adm_restoration_sums`` launch at 3x512x512, crop_border 4, for B = 1 and B = 8, on byte pairs and on a float32 prediction
    against a byte target (what the sampler passes is float32 on both sides: that form too).  Device events around --launches
    back-to-back launches, divided; medians over --reps windows after warm-up, the forms alternating inside one loop so that they share
    whatever else the machine is doing.  The launches are the raw C-ABI call on buffers made once; ``enqueue_ms`` is the host's time per
    call in the same windows, and ``single_launch_ms`` one launch between two events (which adds the events' own cost): the kernel's
    time lies below both;
  * the host half (``metrics_from_sums``) per image, and on this host's CPU the NumPy restatement (tests/restoration_ref.py, the direct
    2-D window) for the whole score of one such image;
  * one sampled image of configs/super-resolution/div2k_cond_ddm_const_ldm.yaml on the synthetic condition encoder (random weights,
    --sample-size pixels square) and the launch's share of it;
  * the worst per-plane SSIM deviation of the kernel from the restatement over the shapes, channel counts, shaves and data families of
    tests/test_hip_restoration_metrics.py, against its bar of 1e-10, and the same at 3x512x512.
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


def worst_deviation(dev):
    """The largest |kernel - restatement| of a per-plane SSIM over the test shapes; SSE words must be equal."""
    import restoration_ref as R
    from adm_amd.metrics.restoration import restoration_sums
    worst, where = 0.0, None
    for hw, B in R.GPU_SHAPES:
        for family in R.FAMILIES:
            for C in (1, 3):
                for s in (0, 4):
                    p, g, want = R.batch_ref(family, hw, B, C, s)
                    sse, ssim = restoration_sums(torch.from_numpy(np.array(p)).to(dev), torch.from_numpy(np.array(g)).to(dev), s)
                    assert np.array_equal(sse.cpu().numpy(), np.stack([R.words(r["sse"]) for r in want])), (hw, family, C, s)
                    gap = float(np.abs(ssim.cpu().numpy() / ((hw[0] - 10) * (hw[1] - 10)) - np.stack([r["ssim_planes"] for r in want])).max())
                    if gap > worst:
                        worst, where = gap, f"{family} {hw[0]}x{hw[1]} B{B} C{C} s{s}"
    return worst, where


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--crop-border", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--launches", type=int, default=50, help="back-to-back launches per timed window")
    ap.add_argument("--sample-size", type=int, default=512)
    ap.add_argument("--skip-sample", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import restoration_ref as R
    from adm_amd import hip
    from adm_amd.metrics.restoration import metrics_from_sums, restoration_sums
    from train_uncond_dpm import Cfg, build_model
    if not torch.cuda.is_available():
        raise RuntimeError("tools/restoration_metrics_cost.py measures the kernel: it needs a GPU")
    hip.lib()
    dev = torch.device("cuda", 0)
    H = W = args.size
    s = args.crop_border
    res = {"what": "restoration score (adm_restoration_sums + host half) on one MI355X; ms = median (min, max) per launch",
           "size": [3, H, W], "crop_border": s, "reps": args.reps, "launches_per_window": args.launches,
           "tile": 32, "blocks_per_image": int(hip.lib().adm_restoration_blocks(H - 2 * s, W - 2 * s))}
    worst, where = worst_deviation(dev)
    res["worst_ssim_deviation_over_test_shapes"] = {"value": worst, "case": where, "bar": R.BAR}
    gen = torch.Generator(device=dev).manual_seed(5)
    for B in (1, 8):
        target = torch.randint(0, 256, (B, 3, H, W), device=dev, dtype=torch.uint8, generator=gen)
        pred = (target.to(torch.int16) + torch.randint(-3, 4, (B, 3, H, W), device=dev, generator=gen).to(torch.int16)).clamp(0, 255).to(torch.uint8)
        forms = {"u8_u8": [pred, target], "f32_u8": [(pred.float() / 255).contiguous(), target],
                 "f32_f32": [(pred.float() / 255).contiguous(), (target.float() / 255).contiguous()]}
        first = None
        for name, (p, g) in forms.items():          # what is timed is what is right: every form gives the bytes' sums
            sse, ssim = restoration_sums(p, g, s)
            if first is None:
                first = (sse, ssim)
            assert torch.equal(sse, first[0]) and torch.equal(ssim, first[1]), name
        if B == 1:
            p, g = pred[0].cpu().numpy(), target[0].cpu().numpy()
            t0 = time.perf_counter()
            want = R.image_ref(p, g, s)
            res["host_numpy_restatement_ms_per_image"] = [round((time.perf_counter() - t0) * 1e3, 1)]
            assert np.array_equal(first[0][0].cpu().numpy(), R.words(want["sse"]))
            count = (H - 2 * s - 10) * (W - 2 * s - 10)
            res["ssim_deviation_at_size"] = float(np.abs(first[1][0].cpu().numpy() / count - want["ssim_planes"]).max())
            words, sums = first[0].cpu().numpy(), first[1].cpu().numpy()
            res["host_half_ms_per_image"] = host_ms(lambda: metrics_from_sums(words, sums, (H - 2 * s, W - 2 * s)), 20)
            res["metrics_at_size"] = metrics_from_sums(words, sums, (H - 2 * s, W - 2 * s))
        P = 4
        blocks = int(hip.lib().adm_restoration_blocks(H - 2 * s, W - 2 * s))
        sse, ssim = torch.empty(B, P, 2, device=dev, dtype=torch.int64), torch.empty(B, P, device=dev, dtype=torch.float64)
        partial, ticket = torch.empty(B, blocks, P, 2, device=dev, dtype=torch.int64), torch.zeros(B, device=dev, dtype=torch.int32)
        raw = lambda p, g: hip.call("adm_restoration_sums", hip.ptr(p), int(p.dtype == torch.float32), hip.ptr(g), int(g.dtype == torch.float32),
                                    hip.ptr(sse), hip.ptr(ssim), hip.ptr(partial), hip.ptr(ticket), B, 3, H, W, s)
        ms, enq, single = {n: [] for n in forms}, {n: [] for n in forms}, {n: [] for n in forms}
        for it in range(args.warmup + args.reps):
            for name, (p, g) in forms.items():
                v, e = window_ms(lambda: raw(p, g), args.launches)
                one, _ = window_ms(lambda: raw(p, g), 1)
                if it >= args.warmup:
                    ms[name].append(v), enq[name].append(e), single[name].append(one)
        assert torch.equal(sse, first[0]) and torch.equal(ssim, first[1]) and not bool(ticket.any())
        for name in forms:
            res[f"launch_ms_B{B}_{name}"] = median3(ms[name])
            res[f"enqueue_ms_B{B}_{name}"] = median3(enq[name])
            res[f"single_launch_ms_B{B}_{name}"] = median3(single[name])
    res["host_cpus_visible"] = os.cpu_count()
    if not args.skip_sample:
        import sample_cond_ldm as S
        scfg = Cfg(yaml.load(open(os.path.join(ROOT, "configs", "super-resolution", "div2k_cond_ddm_const_ldm.yaml")), Loader=yaml.SafeLoader))
        torch.manual_seed(8)
        ldm = build_model(scfg.model).to(dev).eval()
        ldm.model.init_conv_mask = S.SyntheticCondEncoder(getattr(ldm.model, "f_cond", 128)).to(dev)
        n = args.sample_size
        crop, stride = tuple(scfg.sampler.crop_size), tuple(scfg.sampler.stride)
        batch = {"cond": torch.rand(1, 3, n // 4, n // 4, device=dev) * 2 - 1, "ori_size": (n, n)}

        def image():
            with torch.no_grad():
                return S.FORMS["slide_x4"](ldm, scfg.sampler, batch, crop, stride)

        for _ in range(2):
            pred = image()
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            pred = image()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        assert tuple(pred.shape) == (1, 3, n, n) and bool(torch.isfinite(pred).all())
        res["sampled_image_ms"] = median3(ms, 1)
        res["sampled_image"] = {"size": [n, n], "windows": len(S.slide_windows(n // 4, n // 4, crop, stride)),
                                "sampling_timesteps": int(scfg.model.sampling_timesteps), "cond_encoder": "synthetic", "images_timed": len(ms)}
        res["launch_share_of_sampled_image_percent"] = round(100.0 * res["launch_ms_B1_f32_f32"][0] / res["sampled_image_ms"][0], 4)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
