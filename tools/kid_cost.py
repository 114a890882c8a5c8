#!/usr/bin/env python3
"""Cost of the kernel Inception distance on the GPU: one ``adm_kid_sums`` launch for S = 100 subsets of m = 1000 rows at D = 2048,
from synthetic features (n1 = 10 000, n2 = 50 000: the features of 60 000 images, 490 MB, stay on the device).

  python tools/kid_cost.py --out profiles/kid_cost.json

Reports the launch time (device events after warm-up, the median of 20 launches), its rate over the bound the 157 TFLOP/s f32 MFMA
peak sets for 2 m^2 2D FLOP per subset (the symmetric blocks computed once), the time of the path the reference takes on this host
(the features copied to the CPU, then per subset three float32 Gram matrices, their cube and their sums in NumPy), and the launch's
share of the 7.1 s that eval_fid.py spends extracting 50 000 images (profiles/fid_cost.json).  The values of the features do not
change the cost; the index tables are the ones ``kid_indices`` draws.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32_MFMA_PEAK = 157e12


def host_path(f1, f2, idx1, idx2, subsets):
    """seconds for the device -> host copy, and per subset for the float32 NumPy arithmetic the reference does"""
    t0 = time.perf_counter()
    a1, a2 = f1.cpu().numpy(), f2.cpu().numpy()
    copy_s = time.perf_counter() - t0
    D, m = a1.shape[1], idx1.shape[1]
    t0 = time.perf_counter()
    out = np.zeros(subsets)
    for s in range(subsets):
        X, Y = a1[idx1[s]], a2[idx2[s]]
        kxx, kyy, kxy = ((np.matmul(A, B.T) * (1.0 / D) + 1) ** 3 for A, B in ((X, X), (Y, Y), (X, Y)))
        out[s] = ((kxx.sum() - np.trace(kxx) + kyy.sum() - np.trace(kyy)) / (m * (m - 1)) - 2 * kxy.sum() / (m * m))
    return copy_s, (time.perf_counter() - t0) / subsets, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subsets", type=int, default=100)
    ap.add_argument("--subset-size", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--n1", type=int, default=10000)
    ap.add_argument("--n2", type=int, default=50000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--host-subsets", type=int, default=10, help="subsets timed on the host path (scaled to --subsets)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kid_cost.py measures on the GPU; there is none here")
    from adm_amd.metrics import kid
    dev = torch.device("cuda", 0)
    S, m, D = args.subsets, args.subset_size, args.dim
    gen = torch.Generator(device=dev).manual_seed(0)
    f1 = torch.rand(args.n1, D, device=dev, generator=gen).sub_(1.0 / 3.0).clamp_(min=0)
    f2 = torch.rand(args.n2, D, device=dev, generator=gen).sub_(0.3).clamp_(min=0)
    idx1, idx2 = kid.kid_indices(args.n1, args.n2, S, m)
    for _ in range(3):
        sums = kid.kid_sums(f1, f2, idx1, idx2)
    torch.cuda.synchronize()
    # the launch alone: tables and workspace are on the device before the first event
    from adm_amd import hip
    d1, d2 = torch.from_numpy(idx1).to(dev), torch.from_numpy(idx2).to(dev)
    partial = torch.empty(S, int(hip.lib().adm_kid_sums_blocks(m)), device=dev, dtype=torch.float64)
    ms = []
    for _ in range(args.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip.call("adm_kid_sums", hip.ptr(f1), args.n1, hip.ptr(f2), args.n2, D, hip.ptr(d1), hip.ptr(d2), S, m, 3, 1.0 / D, 1.0,
                 hip.ptr(sums), hip.ptr(partial))
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    res_gpu = kid.kid_from_features(f1, f2, S, m)
    torch.cuda.synchronize()
    whole_s = time.perf_counter() - t0
    launch_ms = statistics.median(ms)
    flop = S * 2.0 * m * m * 2.0 * D
    hs = min(args.host_subsets, S)
    copy_s, per_subset_s, host_mmd = host_path(f1, f2, idx1, idx2, hs)
    gpu_mmd = kid.mmd_from_sums(sums, m)[:hs]
    extraction_s = json.load(open(os.path.join(ROOT, "profiles", "fid_cost.json")))["seconds_for_50000_images"]
    res = {"subsets": S, "subset_size": m, "dim": D, "n1": args.n1, "n2": args.n2,
           "launch_ms_median": launch_ms, "launch_ms_min": min(ms), "launch_ms_max": max(ms), "launches": args.launches,
           "kid_from_features_seconds_host_clock": whole_s,
           "tflop": flop / 1e12, "f32_mfma_bound_ms": flop / F32_MFMA_PEAK * 1e3,
           "rate_over_f32_mfma_bound": flop / F32_MFMA_PEAK / (launch_ms * 1e-3),
           "host_copy_seconds": copy_s, "host_numpy_seconds_per_subset": per_subset_s, "host_subsets_timed": hs,
           "host_path_seconds": copy_s + per_subset_s * S, "host_threads": torch.get_num_threads(),
           "host_float32_vs_device_max_abs": float(np.abs(host_mmd - gpu_mmd).max()),
           "share_of_50000_image_extraction": launch_ms * 1e-3 / extraction_s,
           "kid_mean": res_gpu[kid.KEY_KID_MEAN], "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
