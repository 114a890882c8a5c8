#!/usr/bin/env python3
"""Cost of FID / Inception score on the GPU: the InceptionV3 extractor at B = 64 on 32x32 uint8 inputs, the streaming statistics,
and the host sqrtm.

  python tools/fid_cost.py --out profiles/fid_cost.json

Reports images/s of the extractor ('2048' features) from a host clock around synchronised blocks of batches, the extractor's rate
over the f32 MFMA ceiling (the forward's FLOP computed from the layer table, over 157 TFLOP/s: a whole-program figure, not a
kernel's share of peak), the share of each kernel from device events around every launch (a run of its own, events serialise
nothing but add host work), the projected time for 50 000 images including the statistics, and the time of scipy's sqrtm at
D = 2048 on this host's CPU.  The weights are synthetic (tests/inception_ref.py): the cost does not depend on their values.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F32_MFMA_PEAK = 157e12


def forward_flop(inc):
    """multiply-adds x 2 of the real (unpadded) convolutions and the fc at 299x299, per image"""
    def out(n, k, s, p):
        return (n + 2 * p - k) // s + 1
    total, hw = 0, (299, 299)
    for u in inc.STEM:
        if isinstance(u, int):
            hw = (out(hw[0], 3, 2, 0), out(hw[1], 3, 2, 0))
            continue
        _, ci, co, k, s, p = u
        hw = (out(hw[0], k[0], s, p[0]), out(hw[1], k[1], s, p[1]))
        total += 2 * hw[0] * hw[1] * co * ci * k[0] * k[1]
    for _, branches, _ in inc.BLOCKS:
        nxt = hw
        for pool, chain, tails in branches:
            cur = hw
            for u in list(chain) + list(tails):
                _, ci, co, k, s, p = u
                o = (out(cur[0], k[0], s, p[0]), out(cur[1], k[1], s, p[1]))
                total += 2 * o[0] * o[1] * co * ci * k[0] * k[1]
                if u in chain:
                    cur = o
                else:
                    nxt = o
            if not tails and pool == inc.MAX_S2:
                nxt = (out(hw[0], 3, 2, 0), out(hw[1], 3, 2, 0))
        hw = nxt
    return total + 2 * 2048 * 1008


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batches", type=int, default=10, help="batches per timed block")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fid_cost.py measures on the GPU; there is none here")
    import inception_ref as R
    from adm_amd import hip
    from adm_amd.metrics import fid, inception as inc
    dev = torch.device("cuda", 0)
    net = inc.FeatureExtractorInceptionV3(["2048"])
    net.load_state_dict(R.synthetic_state_dict(inc.state_dict_shapes()), strict=True)
    net = net.to(dev)
    imgs = R.images_u8((args.batch, 3, 32, 32), "fid.cost").to(dev)
    for _ in range(2):
        feats = net(imgs)[0]
    torch.cuda.synchronize()
    times = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _ in range(args.batches):
            feats = net(imgs)[0]
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / args.batches)
    per_batch = min(times)
    st = fid.FeatureStats(2048, dev)
    st.update(feats)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.batches):
        st.update(feats)
    torch.cuda.synchronize()
    stats_batch = (time.perf_counter() - t0) / args.batches
    # shares: device events around every launch of one forward
    events, real = [], hip.call

    def timed(name, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real(name, *a)
        e1.record()
        events.append((name, e0, e1))
    hip.call = timed
    try:
        net(imgs)
        st.update(feats)
        torch.cuda.synchronize()
    finally:
        hip.call = real
    by_kernel = {}
    for name, e0, e1 in events:
        by_kernel[name] = by_kernel.get(name, 0.0) + e0.elapsed_time(e1)
    whole = sum(by_kernel.values())
    sg = np.cov(np.random.RandomState(0).randn(4096, 2048), rowvar=False)
    t0 = time.perf_counter()
    fid.fid_from_stats(fid.Stats(np.zeros(2048), sg, 4096), fid.Stats(np.ones(2048) * 0.01, sg * 1.1 + np.eye(2048) * 0.01, 4096))
    sqrtm_s = time.perf_counter() - t0
    flop = forward_flop(inc)
    rate = args.batch / per_batch
    res = {"batch": args.batch, "input": "32x32 uint8", "features": "2048",
           "extractor_images_per_s": rate, "extractor_ms_per_batch": per_batch * 1e3,
           "extractor_ms_per_batch_rounds": [t * 1e3 for t in times],
           "forward_gflop_per_image": flop / 1e9, "f32_mfma_bound_images_per_s": F32_MFMA_PEAK / flop,
           "extractor_rate_over_f32_mfma_bound": rate * flop / F32_MFMA_PEAK,
           "stats_ms_per_batch_D2048": stats_batch * 1e3,
           "seconds_for_50000_images": 50000 / args.batch * (per_batch + stats_batch),
           "kernel_share_of_device_event_time": {k: v / whole for k, v in sorted(by_kernel.items())},
           "kernel_ms_per_batch_device_events": {k: v for k, v in sorted(by_kernel.items())},
           "host_sqrtm_seconds_D2048": sqrtm_s, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
