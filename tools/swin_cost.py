#!/usr/bin/env python3
"""Cost of the Swin-B condition encoder's forward on one MI355X.

  python tools/swin_cost.py --out profiles/swin_cost.json

Times, with HIP events after warm-up (medians of --reps runs):
  * the Swin-B forward at the SR recipe's condition crop (128x128, configs/super-resolution/div2k_cond_ddm_const_ldm.yaml
    sampler.crop_size) for a window batch of --batch crops (16: the batch bench.py --config sr uses) and for one crop;
  * the window attention kernel alone at each stage's grid;
  * one window batch of sample_cond_ldm.py's own path (slide_sample_sr with main()'s sample function) on the full-size model:
    the encoder once, then the 5-step latent sampler, the decode and the stitching -- and the encoder's share of it.
It also counts, for the three kernels of csrc/swin.hip, the bytes a launch requests from memory against the minimum (every input
and output element once).  These counts are analytic (from the kernels' access pattern).  The hardware's own figures come from a
counter pass of its own, merged into the same file afterwards:

  rocprofv3 --pmc FETCH_SIZE WRITE_SIZE -d <dir> --output-format csv -- python tools/swin_cost.py --mode counters
  python tools/swin_cost.py --merge-counters <dir> --out profiles/swin_cost.json          # no GPU needed

(one launch of each kernel at stage 1 of the same batch; FETCH_SIZE / WRITE_SIZE are in KB, and on gfx950 FETCH_SIZE reports
half the bytes of wide coalesced reads -- tools/summarize_profiles.py -- so it is recorded raw next to the analytic count).

  python tools/swin_cost.py --train --out profiles/swin_train_cost.json [--parent-forward-ms MS]

times the TRAINING path instead: the Swin-B forward + backward (enable_training(), stochastic depth off and at the reference's
0.5) for the same window batch, the forward alone of the frozen module, and every backward kernel of csrc/swin.hip at every
stage's shape (window attention with and without shift, LayerNorm, PatchMerging's LayerNorm, row_scale_add).  The file records,
next to these, the forward-only time measured at the parent commit when it is given with --parent-forward-ms (the figure a run of
this tool at that commit printed as encoder_forward_ms.batch_<B>); null until then.

The weights are the default initialisation (the cost does not depend on their values; nothing is fetched).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)


def ceil7(n):
    return -(-n // 7) * 7


def attn_bytes(B, H, W, C, heads):
    """requested: q, k, v of every real token once (a token belongs to one window), the qkv bias in place of every padding token's
    k and v, the head's column of the bias table once per (window, head), the output once."""
    Ph, Pw = ceil7(H), ceil7(W)
    units = B * (Ph // 7) * (Pw // 7) * heads
    real, pad = B * H * W, B * (Ph * Pw - H * W)
    moved = 4 * (real * 3 * C + pad * 2 * C + units * 169 + real * C)
    minimal = 4 * (real * 3 * C + 3 * C + 169 * heads + real * C)
    return moved, minimal


def stage1_launches(B, crop):
    """(name, kernel-name fragment, analytic bytes requested, minimal bytes) of the counter pass's three launches."""
    g, C, heads = crop // 4, 128, 4
    M, Mo = B * g * g, B * ((g + 1) // 2) ** 2
    a_req, a_min = attn_bytes(B, g, g, C, heads)
    return [("swin_attn_fwd", "swin_attn_kernel", a_req, a_min),
            ("ln_affine_fwd", "ln_affine_kernelILb0", 4 * (2 * M * C + 2 * M * C), 4 * (2 * M * C + 2 * C)),
            ("swin_merge_ln_fwd", "ln_affine_kernelILb1", 4 * (M * C + Mo * 4 * C + 2 * Mo * 4 * C), 4 * (M * C + Mo * 4 * C + 8 * C))]


def merge_counters(d, out, B, crop):
    files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *counter_collection.csv under {d}")
    rows = [r for f in files for r in csv.DictReader(open(f))]
    res = json.load(open(out))
    meas = {}
    for name, frag, req, minimal in stage1_launches(B, crop):
        ent = {"bytes_requested_analytic": req, "bytes_minimal": minimal, "launches_counted": 0}
        for r in rows:
            if frag in r["Kernel_Name"].replace("<", "I").replace("false", "Lb0").replace("true", "Lb1").replace("(bool)", ""):
                key = r["Counter_Name"] + "_KB"
                ent[key] = round(ent.get(key, 0.0) + float(r["Counter_Value"]), 3)
                ent["launches_counted"] += r["Counter_Name"] == "FETCH_SIZE"
        meas[name] = ent
    res["measured_counters_stage1"] = {"batch": B, "note": "rocprofv3 --pmc FETCH_SIZE WRITE_SIZE, one launch each, raw KB "
                                       "(gfx950 FETCH_SIZE reports half the bytes of wide coalesced reads)", "kernels": meas}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["measured_counters_stage1"]))


def counters_pass(B, crop):
    from adm_amd import hip, ops_swin as osw
    hip.lib()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    g, C, heads = crop // 4, 128, 4
    qkv = torch.randn(B, g, g, 3 * C, device=dev, generator=gen)
    x = torch.randn(B, g, g, C, device=dev, generator=gen)
    w, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    w4, b4 = torch.ones(4 * C, device=dev), torch.zeros(4 * C, device=dev)
    tab = torch.zeros(169, heads, device=dev)
    torch.cuda.synchronize()
    osw.window_attention(qkv, torch.zeros(3 * C, device=dev), tab, heads, 3)
    osw.layer_norm(x, w, b)
    osw.merge_layer_norm(x, w4, b4)
    torch.cuda.synchronize()
    print("counter pass: one launch of each kernel done")


def train_cost(args):
    from adm_amd import hip, ops_swin as osw
    from adm_amd.unet.swin_transformer import swin_b
    hip.lib()
    dev = torch.device("cuda", 0)
    torch.manual_seed(7)
    gen = torch.Generator(device=dev).manual_seed(1)
    B, g = args.batch, args.crop // 4
    x = torch.rand(B, 3, args.crop, args.crop, device=dev, generator=gen) * 2 - 1
    res = {"what": "Swin-B condition encoder, training path (f32, HIP kernels), one MI355X; ms = median (min, max) of HIP-event timings",
           "crop": [args.crop, args.crop], "batch": B, "reps": args.reps,
           "forward_only_ms_at_parent_commit": args.parent_forward_ms, "forward_backward_ms": {}, "backward_kernels_ms": []}
    frozen = swin_b().to(dev).eval()
    res["forward_only_ms_frozen"] = timed(lambda: frozen(x), args.warmup, args.reps)
    del frozen
    enc = swin_b().to(dev)
    for tag, p in (("stochastic_depth_0", 0.0), ("stochastic_depth_0.5", None)):
        enc.enable_training(p).train()

        def step():
            for q in enc.parameters():
                q.grad = None
            feats = enc(x)
            torch.autograd.backward(feats, [torch.ones_like(f) for f in feats])

        res["forward_backward_ms"][tag] = timed(step, args.warmup, args.reps)
        res["forward_backward_ms"][tag + "_forward_part"] = timed(lambda: enc(x), args.warmup, args.reps)
    del enc
    one = lambda *s: torch.randn(*s, device=dev, generator=gen)
    for st, (heads, depth) in enumerate(zip((4, 8, 16, 32), (2, 2, 18, 2))):
        H = W = -(-g // 2 ** st)
        C = 128 * 2 ** st
        ent = {"stage": st + 1, "grid": [H, W], "C": C, "heads": heads, "batch": B, "blocks_in_stage": depth}
        qkv, qb, tab, do = one(B, H, W, 3 * C), one(3 * C) * 0.1, one(169, heads) * 0.1, one(B, H, W, C)
        dq, dt, db = torch.empty_like(qkv), torch.empty_like(tab), torch.empty_like(qb)
        ws = torch.empty(hip.lib().adm_swin_attn_bwd_ws_floats(B, H, W, heads), device=dev)
        for shift in (0, 3):
            ent[f"swin_attn_bwd_shift{shift}"] = timed(lambda: hip.call(
                "adm_swin_attn_bwd", hip.ptr(qkv), hip.ptr(qb), hip.ptr(tab), hip.ptr(do), hip.ptr(dq), hip.ptr(dt), hip.ptr(db), hip.ptr(ws),
                B, H, W, C, heads, 7, shift, shift, 0, 0), args.warmup, args.reps)
            ent[f"swin_attn_fwd_shift{shift}"] = timed(lambda: osw.window_attention(qkv, qb, tab, heads, shift), args.warmup, args.reps)
        xs, w, dy, dx = one(B, H, W, C), torch.ones(C, device=dev), one(B, H, W, C), torch.empty(B, H, W, C, device=dev)
        dw, dbb = torch.empty(C, device=dev), torch.empty(C, device=dev)
        ws = torch.empty(hip.lib().adm_ln_bwd_ws_floats(B * H * W, C), device=dev)
        ent["ln_affine_bwd"] = timed(lambda: hip.call("adm_ln_affine_bwd", hip.ptr(xs), hip.ptr(w), hip.ptr(dy), hip.ptr(dx), hip.ptr(dw),
                                                      hip.ptr(dbb), hip.ptr(ws), B * H * W, C, 1e-5, 0), args.warmup, args.reps)
        s = torch.ones(B, device=dev)
        ent["rowscale_add"] = timed(lambda: hip.call("adm_rowscale_add", hip.ptr(xs), hip.ptr(dy), hip.ptr(s), hip.ptr(dx), B, H * W * C),
                                    args.warmup, args.reps)
        if st < 3:
            Ho, Wo = (H + 1) // 2, (W + 1) // 2
            w4, dy4 = torch.ones(4 * C, device=dev), one(B, Ho, Wo, 4 * C)
            dw4, db4 = torch.empty(4 * C, device=dev), torch.empty(4 * C, device=dev)
            ws = torch.empty(hip.lib().adm_ln_bwd_ws_floats(B * Ho * Wo, 4 * C), device=dev)
            ent["swin_merge_ln_bwd"] = timed(lambda: hip.call("adm_swin_merge_ln_bwd", hip.ptr(xs), hip.ptr(w4), hip.ptr(dy4), hip.ptr(dx),
                                                              hip.ptr(dw4), hip.ptr(db4), hip.ptr(ws), B, H, W, C, 1e-5, 0),
                                             args.warmup, args.reps)
        res["backward_kernels_ms"].append(ent)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true", help="time the training path (forward + backward and every backward kernel)")
    ap.add_argument("--parent-forward-ms", type=float, default=None,
                    help="with --train: the forward-only time measured at the parent commit, recorded next to the new figures")
    ap.add_argument("--mode", choices=["time", "counters"], default="time")
    ap.add_argument("--merge-counters", default=None, help="directory of a rocprofv3 --pmc pass; merged into --out (no GPU needed)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--crop", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--skip-sampler", action="store_true", help="encoder and kernels only (no full-size SR model)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.merge_counters:
        return merge_counters(args.merge_counters, args.out, args.batch, args.crop)
    if args.mode == "counters":
        return counters_pass(args.batch, args.crop)
    if args.train:
        return train_cost(args)

    from adm_amd import hip, ops_swin as osw
    from adm_amd.unet.swin_transformer import swin_b
    hip.lib()
    dev = torch.device("cuda", 0)
    torch.manual_seed(7)
    enc = swin_b().to(dev).eval()
    res = {"what": "Swin-B condition encoder forward (f32, HIP kernels), one MI355X; ms = median (min, max) of HIP-event timings",
           "crop": [args.crop, args.crop], "reps": args.reps, "encoder_forward_ms": {}, "attention_kernel_ms": [], "bytes": {}}
    gen = torch.Generator(device=dev).manual_seed(1)
    for B in sorted({1, args.batch}):
        x = torch.rand(B, 3, args.crop, args.crop, device=dev, generator=gen) * 2 - 1
        res["encoder_forward_ms"][f"batch_{B}"] = timed(lambda: enc(x), args.warmup, args.reps)
    B = args.batch
    g = args.crop // 4
    for st, (heads, depth) in enumerate(zip((4, 8, 16, 32), (2, 2, 18, 2))):
        H = W = -(-g // 2 ** st)
        C = 128 * 2 ** st
        qkv = torch.randn(B, H, W, 3 * C, device=dev, generator=gen)
        qb = torch.randn(3 * C, device=dev, generator=gen) * 0.1
        tab = torch.randn(169, heads, device=dev, generator=gen) * 0.1
        moved, minimal = attn_bytes(B, H, W, C, heads)
        for shift in (0, 3):
            ms = timed(lambda: osw.window_attention(qkv, qb, tab, heads, shift), args.warmup, args.reps)
            res["attention_kernel_ms"].append({"stage": st + 1, "grid": [H, W], "C": C, "heads": heads, "shift": shift, "batch": B,
                                               "blocks_in_stage": depth, "ms": ms, "bytes_requested": moved, "bytes_minimal": minimal,
                                               "GB_per_s_at_median": round(moved / ms[0] / 1e6, 1)})
        # LayerNorm of the stage and the PatchMerging that follows it
        M = B * H * W
        res["bytes"][f"ln_affine_stage{st + 1}"] = {"rows": M, "C": C, "bytes_requested": 4 * (2 * M * C + 2 * M * C),
                                                    "bytes_minimal": 4 * (2 * M * C + 2 * C),
                                                    "note": "weight and bias are re-read by every row (from cache)"}
        if st < 3:
            Mo = B * ((H + 1) // 2) * ((W + 1) // 2)
            res["bytes"][f"merge_ln_stage{st + 1}"] = {"in": [B, H, W, C], "bytes_requested": 4 * (M * C + Mo * 4 * C + 2 * Mo * 4 * C),
                                                       "bytes_minimal": 4 * (M * C + Mo * 4 * C + 8 * C)}
    if not args.skip_sampler:
        # sample_cond_ldm.py's own path: slide_sample_sr over one condition image whose windows form one batch of --batch crops,
        # with main()'s sample function (the encoder once per window batch, then the 5-step sampler and the decode)
        import bench
        from sample_cond_ldm import slide_sample_sr, slide_windows
        ldm = bench.build_sr_model(dev).eval()
        ldm.model.init_conv_mask = enc
        n = max(1, int(round(B ** 0.5)))
        side = args.crop + (args.crop // 2) * (n - 1)
        crop, stride = (args.crop, args.crop), (args.crop // 2, args.crop // 2)
        nwin = len(slide_windows(side, side, crop, stride))
        cond = torch.rand(1, 3, side, side, device=dev, generator=gen) * 2 - 1
        down = ldm.first_stage_model.down_ratio
        marks = []

        def fn(c):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            feats = list(ldm.model.init_conv_mask(c))
            e1.record()
            marks.append((e0, e1))
            return ldm.sample(cond=feats, latent_hw=(c.shape[2] * 4 // down, c.shape[3] * 4 // down))

        run = lambda: slide_sample_sr(fn, cond, (4 * side, 4 * side), crop, stride, window_batch=0)
        t_all = timed(run, 1, max(3, args.reps // 3))
        torch.cuda.synchronize()
        enc_ms = sorted(a.elapsed_time(b) for a, b in marks[1:])          # (the warm-up call's mark is dropped)
        t_e = round(statistics.median(enc_ms), 4)
        res["sr_window_batch"] = {"condition_image": [side, side], "windows_in_the_batch": nwin, "sampling_timesteps": 5,
                                  "slide_sample_sr_ms": t_all, "encoder_ms_inside_it": [t_e, round(enc_ms[0], 4), round(enc_ms[-1], 4)],
                                  "encoder_share_percent": round(100.0 * t_e / t_all[0], 2),
                                  "note": "sample_cond_ldm.slide_sample_sr with main()'s sample function on the full-size SR model"}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
