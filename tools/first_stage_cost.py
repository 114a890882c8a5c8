#!/usr/bin/env python3
"""Cost of training the first stage of each conditional recipe on one MI355X: the batch source next to the two micro-steps it feeds.

  python tools/first_stage_cost.py --out profiles/first_stage_cost.json

Recipes (the committed YAMLs, on their synthetic pools; fp32):
  duts    configs/saliency/duts_ae_kl_384x384.yaml                 1 x 384 x 384, B = 8   (adm_image_resize_batch, C = 1)
  sketch  configs/sketch2img/sketchcoco_ae_kl_256x256_d4.yaml      3 x 256 x 256, B = 8   (adm_image_resize_batch, C = 3)
  div2k   configs/super-resolution/div2k_ae_kl_512x512_d4.yaml     3 x 512 x 512, B = 4   (adm_sr_batch: its HR crop)

Per recipe, all from device events:
  * the batch: the kernel alone on fixed draws, and the stream's whole batch with its draws made on the device (ms = median (min,
    max) of --reps launches after warm-up);
  * the autoencoder and the discriminator micro-step, AdamW steps included: blocks of --steps micro-steps of each kind alternate
    --rounds times in one call, after a warm-up of every shape (tools/ae_train_cost.py's scheme).
Comparisons, each alternated with what it is compared to in the same call:
  * the one-plane batch against adm_pair_resize_batch making BOTH planes for the same draws from pools of the same sizes -- the
    code that existed; the one-plane launch does a subset of that launch's work (duts: the map of the pair; sketch: the photo);
  * the one-plane batch against PIL in one process on this host (Image.resize, the flip, ToTensor, *2-1); null without PIL;
  * the one-channel step against the three-channel step at the same size (1 x 384 x 384 against 3 x 384 x 384, B = 8).
Shares of the step, from the same operators timed in isolation at the step's shapes (forward + backward under autograd for the
autoencoder micro-step, whose two mid blocks both run them; forward only for the discriminator micro-step's two no-grad passes):
  * the three convs whose one real channel is padded to 32: encoder.conv_in, decoder.conv_out, discriminator conv 0 (duts);
  * the mid-block attention at L = 9216 (duts, 96 x 96 tokens) and at L = 16384 (div2k, 128 x 128 tokens).
The LPIPS weights are synthetic (tools/lpips_cost.py synthetic_lpips); weights are the default initialisation and the images
U(0,255): the cost depends on neither.  global_step is past disc_start, so the discriminator contributes to both micro-steps."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

RECIPES = {"duts": "configs/saliency/duts_ae_kl_384x384.yaml", "sketch": "configs/sketch2img/sketchcoco_ae_kl_256x256_d4.yaml",
           "div2k": "configs/super-resolution/div2k_ae_kl_512x512_d4.yaml"}


def alternated(fns, warmup, reps):
    """{name: [median, min, max] ms} of single calls, the candidates taking turns rep by rep (device events)."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}


def block_ms(fn, n):
    """ms per call of n calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def rounds_ms(kinds, warmup, steps, rounds):
    """{name: {'ms_per_step': [per round], 'mean_ms', 'spread_ms'}}: blocks of `steps` calls of each kind, alternated."""
    for fn in kinds.values():
        block_ms(fn, warmup)
    ms = {k: [] for k in kinds}
    for _ in range(rounds):
        for k, fn in kinds.items():
            ms[k].append(round(block_ms(fn, steps), 3))
    return {k: {"ms_per_step": v, "mean_ms": round(sum(v) / len(v), 3), "spread_ms": round(max(v) - min(v), 3)} for k, v in ms.items()}


def pil_ms(pool, idx, flip, reps):
    """The same batch through PIL in one process on this host: [median, min, max] ms, or None without PIL."""
    try:
        from PIL import Image
    except ImportError:
        return None
    flat, off, hw, C = pool.flat.cpu().numpy(), pool.off.cpu().numpy(), pool.hw_host, pool.channels
    H, W = pool.out_hw
    src = []
    for n in idx:
        h, w = int(hw[n, 0]), int(hw[n, 1])
        src.append(flat[off[n]:off[n] + h * w * C].reshape((h, w, 3) if C == 3 else (h, w)))
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = []
        for a, f in zip(src, flip):
            im = Image.fromarray(a).resize((W, H), Image.BILINEAR)
            if f:
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            t = torch.from_numpy(np.array(im).reshape(H, W, C)).permute(2, 0, 1).float().div(255) * 2 - 1
            out.append(t)
        torch.stack(out)
        ms.append((time.perf_counter() - t0) * 1e3)
    return [round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)]


def build_ae(ddconfig, lossconfig, dev):
    from adm_amd.ddm.encoder_decoder import AutoencoderKL
    from lpips_cost import synthetic_lpips
    torch.manual_seed(0)
    ae = AutoencoderKL(dict(ddconfig), dict(lossconfig, disc_start=0), 3).to(dev)
    ae.enable_training(lpips=synthetic_lpips()).train()
    ae_params = (list(ae.encoder.parameters()) + list(ae.decoder.parameters()) + list(ae.quant_conv.parameters())
                 + list(ae.post_quant_conv.parameters()))
    opts = [torch.optim.AdamW(ae_params, lr=5e-6), torch.optim.AdamW(ae.loss.discriminator.parameters(), lr=5e-6)]
    return ae, opts


def micro_steps(ae, opts, batches):
    def micro(idx):
        def run(it):
            for o in opts[idx:]:
                o.zero_grad(set_to_none=True)
            _, log = ae.training_step(batches[it & 1], idx, 10 + it, loss_scale=0.5)
            opts[idx].step()
            return log
        return run
    return {"ae_micro_step": micro(0), "disc_micro_step": micro(1)}


def fwd_bwd(module_fn, x):
    """(forward-only fn, forward + backward fn) of y = module_fn(x) on a fixed NHWC input, gradients to x and the parameters."""
    xg = x.clone().requires_grad_(True)
    dy = None

    def fwd(_):
        with torch.no_grad():
            module_fn(x)

    def both(_):
        nonlocal dy
        y = module_fn(xg)
        if dy is None:
            dy = torch.randn_like(y)
        y.backward(dy)
    return fwd, both


def attention_share(ae, B, hw, step, args):
    """The mid attention block at the step's shape in isolation, and its share of the two micro-steps: the encoder's and the
    decoder's block both run forward + backward in the autoencoder micro-step and forward in the discriminator micro-step."""
    blk = ae.encoder.mid.attn_1
    C = blk.in_channels
    x = torch.randn(B, hw[0] // 4, hw[1] // 4, C, device=next(ae.parameters()).device)
    fwd, both = fwd_bwd(blk, x)
    t = rounds_ms({"forward": fwd, "forward_backward": both}, 1, args.steps, args.rounds)
    for p in blk.parameters():
        p.grad = None
    return {"tokens": (hw[0] // 4) * (hw[1] // 4), "channels": C, "batch": B, "blocks_per_step": 2,
            "forward_ms": t["forward"], "forward_backward_ms": t["forward_backward"],
            "share_of_ae_micro_step_percent": round(100 * 2 * t["forward_backward"]["mean_ms"] / step["ae_micro_step"]["mean_ms"], 2),
            "share_of_disc_micro_step_percent": round(100 * 2 * t["forward"]["mean_ms"] / step["disc_micro_step"]["mean_ms"], 2)}


def padded_conv_share(ae, B, hw, step, args):
    """encoder.conv_in (1 -> ch), decoder.conv_out (ch -> 1) and the discriminator's conv 0 (1 -> 64, 4x4 stride 2) in isolation: the
    one real channel travels as 32.  conv_in and conv_out run forward + backward in the autoencoder micro-step and forward in the
    discriminator's; conv 0 runs forward + backward in the autoencoder micro-step (without its weight gradient there: the figure
    timed here, with it, is an upper bound) and twice forward + backward in the discriminator's."""
    from adm_amd import ops_ae
    from adm_amd.ddm.encoder_decoder import _conv
    dev = next(ae.parameters()).device
    H, W = hw
    ch = ae.encoder.ch
    d0 = ae.loss.discriminator.main[0]
    ops = {"encoder.conv_in": (lambda x: _conv(ae.encoder.conv_in, x), torch.randn(B, H, W, 32, device=dev)),
           "decoder.conv_out": (lambda x: _conv(ae.decoder.conv_out, x), torch.randn(B, H, W, ch, device=dev)),
           "discriminator.conv0": (lambda x: ops_ae.conv2d_down(x, d0.weight, d0.bias, stride=2, pad_lo=1, pad_hi=1),
                                   torch.randn(B, H, W, 32, device=dev))}
    kinds = {}
    for k, (fn, x) in ops.items():
        kinds[k + ".forward"], kinds[k + ".forward_backward"] = fwd_bwd(fn, x)
    t = rounds_ms(kinds, 1, args.steps, args.rounds)
    for m in (ae.encoder.conv_in, ae.decoder.conv_out, d0):
        for p in m.parameters():
            p.grad = None
    m = lambda k: t[k]["mean_ms"]
    ae_ms = m("encoder.conv_in.forward_backward") + m("decoder.conv_out.forward_backward") + m("discriminator.conv0.forward_backward")
    disc_ms = m("encoder.conv_in.forward") + m("decoder.conv_out.forward") + 2 * m("discriminator.conv0.forward_backward")
    return {"ms": t, "share_of_ae_micro_step_percent": round(100 * ae_ms / step["ae_micro_step"]["mean_ms"], 2),
            "share_of_disc_micro_step_percent": round(100 * disc_ms / step["disc_micro_step"]["mean_ms"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recipes", default="duts,sketch,div2k")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20, help="timed launches of each batch source")
    ap.add_argument("--steps", type=int, default=3, help="micro-steps per timed block")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from adm_amd import hip
    from adm_amd.ddm.image_data import ImageBatchStream, image_batch
    from adm_amd.ddm.pair_data import PairPool, pair_batch
    from adm_amd.ddm.sr_data import sr_batch
    from train_uncond_dpm import Cfg
    from train_vae import check_channels, first_stage_stream
    if not torch.cuda.is_available():
        raise SystemExit("first_stage_cost.py measures on a GPU; none is visible")
    hip.lib()
    dev = torch.device("cuda", 0)
    res = {"what": "first-stage training of the conditional recipes on one MI355X, fp32; device events; batch ms = median (min, max) "
                   f"of {args.reps} launches, candidates alternated; step ms = {args.rounds} rounds of {args.steps} micro-steps per kind, "
                   "alternated in one call, AdamW steps included",
           "host_cpus_visible": os.cpu_count(), "recipes": {}}
    for name in args.recipes.split(","):
        cfg = Cfg(yaml.load(open(os.path.join(ROOT, RECIPES[name])), Loader=yaml.SafeLoader))
        B = int(cfg.data.batch_size)
        size = tuple(cfg.data.get("image_size") or cfg.model.ddconfig.resolution)
        stream = first_stage_stream(cfg.data, B, size, dev, seed=1000)
        check_channels(stream.channels, cfg.model)
        r = {"yaml": RECIPES[name], "batch": B, "channels": stream.channels, "size": list(size),
             "output_MB_per_batch": round(B * stream.channels * size[0] * size[1] * 4 / 1e6, 2)}
        if isinstance(stream, ImageBatchStream):
            pool = stream.pool
            idx, flip = stream.draw()
            r.update(entry="adm_image_resize_batch", pool_images=pool.n, pool_bytes=pool.nbytes,
                     source_sizes=sorted({(int(h), int(w)) for h, w in pool.hw_host}), resize_tables=len(pool.tables["keys"]))
            # the pair launch that existed: both planes for the same draws, from pools of the same source sizes
            pairs = PairPool.from_uniform_draws([tuple(s) for s in pool.hw_host.tolist()], size, dev, stream.gen)
            t = alternated({"one_plane_kernel": lambda: image_batch(pool, idx, flip),
                            "pair_kernel_both_planes": lambda: pair_batch(pairs, idx, flip),
                            "stream_with_device_draws": lambda: next(stream)}, args.warmup, args.reps)
            r["batch_kernel_ms"], r["stream_ms_per_batch_with_device_draws"] = t["one_plane_kernel"], t["stream_with_device_draws"]
            r["pair_kernel_both_planes_ms"] = t["pair_kernel_both_planes"]
            r["one_plane_over_pair"] = round(t["one_plane_kernel"][0] / t["pair_kernel_both_planes"][0], 3)
            if r["one_plane_over_pair"] > 1.0:
                r["one_plane_slower_than_pair_note"] = (
                    "the one-plane launch resizes a subset of the pair launch's planes with the same code; both are a few tens of "
                    "microseconds, where the launch itself and the event pair around it dominate: see the (min, max) of the two")
            r["host_pil_ms_per_batch_one_process"] = pil_ms(pool, idx.tolist(), flip.tolist(), max(3, args.reps // 4))
        else:
            d = stream.draw()
            r.update(entry="adm_sr_batch (the HR crop is the batch's image)", pool_images=stream.pool.n)
            t = alternated({"kernel": lambda: sr_batch(stream.pool, stream.rs, *d), "stream": lambda: next(stream)}, args.warmup, args.reps)
            r["batch_kernel_ms"], r["stream_ms_per_batch_with_device_draws"] = t["kernel"], t["stream"]
        if not args.skip_train:
            ae, opts = build_ae(cfg.model.ddconfig, cfg.model.lossconfig, dev)
            batches = [next(stream)["image"] for _ in range(2)]
            kinds = micro_steps(ae, opts, batches)
            if name == "duts":          # the three-channel step at the same size, alternated with the one-channel step
                dd3 = dict(cfg.model.ddconfig, in_channels=3, out_ch=3)
                ae3, opts3 = build_ae(dd3, dict(cfg.model.lossconfig, disc_in_channels=3), dev)
                b3 = [b.expand(-1, 3, -1, -1).contiguous() for b in batches]
                kinds.update({k + "_three_channels": v for k, v in micro_steps(ae3, opts3, b3).items()})
            step = rounds_ms(kinds, args.warmup, args.steps, args.rounds)
            log = kinds["ae_micro_step"](99)
            assert all(bool(torch.isfinite(v).all()) for v in log.values())
            r["step"] = step
            pair = step["ae_micro_step"]["mean_ms"] + step["disc_micro_step"]["mean_ms"]
            r["images_per_s_for_the_pair"] = round(B / (pair * 1e-3), 2)
            r["batch_share_of_the_pair_percent"] = round(100 * r["stream_ms_per_batch_with_device_draws"][0] / pair, 4)
            if name == "duts":
                pair3 = step["ae_micro_step_three_channels"]["mean_ms"] + step["disc_micro_step_three_channels"]["mean_ms"]
                r["one_channel_over_three_channel_pair"] = round(pair / pair3, 4)
                del ae3, opts3, b3
                r["padded_one_channel_convs"] = padded_conv_share(ae, B, size, step, args)
            if name in ("duts", "div2k"):
                r["mid_attention"] = attention_share(ae, B, size, step, args)
            del ae, opts, batches, kinds
            torch.cuda.empty_cache()
        res["recipes"][name] = r
        print(name, json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
