#!/usr/bin/env python3
"""MI355X counterpart of the reference's conditional latent sampler (/root/reference/sample_cond_ldm.py): super-resolution by
SLIDING-WINDOW sampling with overlap averaging (reference :281-330, `slide_sample_sr`).

``python sample_cond_ldm.py --cfg <yaml>`` builds unet (unet.cond_unet.Unet / unet.cond_unet_sd.Unet) + frozen first stage +
ddm.ddm_const.LatentDiffusion from the YAML exactly as the reference does (:53-66), loads ``sampler.ckpt_path`` (EMA weights
when ``sampler.use_ema``, prefix stripped, :135-147), then for every low-resolution condition image cuts windows of
``sampler.crop_size`` at ``sampler.stride`` (origins clamped to the border, :296-301), samples each window's 4x larger
output crop with the ``sampling_timesteps``-step sampler conditioned on the window, and averages overlapping outputs.

What differs from the reference:
  * windows are sampled in BATCHES (``sampler.window_batch``, default all windows of an image at once) instead of one
    ``model.sample(batch_size=1)`` call per window: each window's trajectory is independent, so batching changes only which
    random draws a window receives, and keeps the GPU full; ``window_batch: 1`` reproduces the reference's call pattern;
  * the condition encoder: ``sampler.cond_encoder: swin_b`` selects the built-in Swin-B (adm_amd.unet.swin_transformer, forward
    only); it is attached before the checkpoint is loaded, so the checkpoint's ``init_conv_mask.*`` tensors (or those of its EMA
    copy) load into it -- no ImageNet weight file is ever fetched, and a checkpoint without them is refused.  Otherwise
    ``sampler.cond_encoder`` names a callable ``module:attr`` that maps a condition crop [B,3,h,w] to the four feature maps
    the denoiser consumes; ``synthetic`` selects a parameter-free pooled pyramid (smoke runs / benchmarking only);
  * every rank handles a disjoint share of the images; no collectives.

With ``data.class_name: ddm.data.InpaintDataset`` (in-painting, configs/inpainting/celebahq_cond_ddm_const_ldm_sample.yaml) there is no
window: each image gets a mask drawn on the device (adm_amd.ddm.inpaint_data), the model is sampled once on the masked image with
``mask=`` / ``cond_image=``, and the composite -- kept pixels from the image, holes from the sample -- is written under the image's
name; ``sampler.save_masks: True`` also writes ``masks/<name>``.  PSNR is printed as the reference's sampler prints it (:195, 217).

With ``data.class_name: ddm.data.DUTSDataset`` and ``split: test`` (saliency, configs/saliency/duts_cond_ddm_const_ldm_sample.yaml) the
condition is the photo resized to the model's resolution and the windows run at the output's own scale (the reference's
``slide_sample``, :220-283: ``slide_sample_sr`` with ``scale=1``); ``sampler.out_channels`` defaults to 1, ``crop_size`` / ``stride`` to
``image_size``; each one-channel prediction is written as a mode-L png under the photo's name, and the PSNR is against the resized map.
``sampler.cal_saliency: True`` (off by default; ``sampler.saliency_normalize``, default True) also scores the prediction's bytes against
the resized map's bytes with adm_amd.metrics.saliency (MAE, F-, S- and E-measure): printed at the end and written to
``<save_folder>/saliency_metrics.json``; on any other data set the key raises.

``sampler.cal_restoration: True`` (off by default) scores the super-resolution and the in-painting predictions -- the dataset entries
with a PSNR line and a colour output -- with adm_amd.metrics.restoration: PSNR and SSIM on RGB and on the Y channel of the BYTES the
png holds (the float prediction is quantised in the kernel as ``save_prediction`` quantises it) against the bytes of the part of
'image' the prediction covers, with ``sampler.restoration_crop_border`` pixels shaved from every side (default 4 for x4
super-resolution, 0 for in-painting, whose composite is scored whole).  Printed at the end and written to
``<save_folder>/restoration_metrics.json``; on any other data set the key raises.  The PSNR line above is untouched.

With ``data.class_name: ddm.data.SketchDataset`` and ``split: test`` (sketch-to-image,
configs/sketch2img/sketchcoco_cond_ddm_const_ldm_sample.yaml) the condition is the ONE-channel sketch resized to ``image_size`` and the
output a three-channel image, sampled in one window and written under the sketch's file name.  No PSNR is printed: a generated
photo has no ground truth to score.

With ``data.class_name: ddm.data.NYUDv2DepthDataset`` and ``split: test`` (depth estimation,
configs/depth_estimation/nyud_cond_ddm_const_ldm_sample.yaml) the condition is the whole 426x560 boxed photo, sampled in overlapping
windows of ``sampler.crop_size`` at ``sampler.stride`` (2 x 3 windows of 320x320 at stride 160), each twice with ``flip_test``.  The
one-channel prediction is a depth fraction (1.0 = 10 m): it is written as a 16-BIT png of round(clip(p, 0, 1) * 10000) under the
photo's name -- the reference writes 8 bits through save_image; ``sampler.depth_png8: True`` keeps that -- and scored against the
ground truth with adm_amd.metrics.depth (abs-rel, RMSE, delta ...): printed at the end and written to
``<save_folder>/depth_metrics.json``.

Which of these a data section selects, and what differs between them, is the ``sampling`` column of adm_amd.ddm.datasets.DATASETS;
``main`` is one loop over that entry.  ``class_name: synthetic`` + ``synthetic_of`` selects the sketch and the depth entries only:
with any other ``synthetic_of`` the items are CondStream's super-resolution pairs.
"""
import argparse
import importlib
import os
import sys
import time

import torch
import yaml

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from adm_amd.ddm.datasets import DATASETS, SR_SAMPLING, sampling_dataset  # noqa: E402
from train_uncond_dpm import Cfg, build_model  # noqa: E402
from sample_uncond import load_weights  # noqa: E402


def slide_windows(h_cond, w_cond, crop, stride):
    """(y1, y2, x1, x2) of every window, in the reference's order (sample_cond_ldm.py:288-301)."""
    (hc, wc), (hs, ws) = crop, stride
    hg = max(h_cond - hc + hs - 1, 0) // hs + 1
    wg = max(w_cond - wc + ws - 1, 0) // ws + 1
    out = []
    for hi in range(hg):
        for wi in range(wg):
            y2 = min(hi * hs + hc, h_cond); x2 = min(wi * ws + wc, w_cond)
            out.append((max(y2 - hc, 0), y2, max(x2 - wc, 0), x2))
    return out


@torch.no_grad()
def slide_sample_sr(sample_fn, cond, image_hw, crop_size, stride, out_channels=3, scale=4, ori_size=None, window_batch=0,
                    flip_test=False):
    """cond [B,C,h,w] -> [B,out_channels,H,W]: mean over the windows covering each output pixel of sample_fn(window) (the 4x
    larger crop).  Windows of equal size are stacked along the batch axis, `window_batch` at a time (0 = all)."""
    B = cond.shape[0]
    H, W = image_hw
    preds = torch.zeros((B, out_channels, H, W), device=cond.device, dtype=torch.float32)
    count = torch.zeros((1, 1, H, W), device=cond.device, dtype=torch.float32)
    wins = slide_windows(cond.shape[2], cond.shape[3], crop_size, stride)
    step = len(wins) if window_batch <= 0 else window_batch
    for i in range(0, len(wins), step):
        chunk = wins[i:i + step]
        crops = torch.cat([cond[:, :, y1:y2, x1:x2] for (y1, y2, x1, x2) in chunk], dim=0).contiguous()
        out = sample_fn(crops).to(torch.float32)
        if flip_test:          # reference :307-310: average with the sample of the mirrored condition, mirrored back
            out = 0.5 * out + 0.5 * sample_fn(crops.flip(dims=[-1])).to(torch.float32).flip(dims=[-1])
        for k, (y1, y2, x1, x2) in enumerate(chunk):
            preds[:, :, y1 * scale:y2 * scale, x1 * scale:x2 * scale] += out[k * B:(k + 1) * B]
            count[:, :, y1 * scale:y2 * scale, x1 * scale:x2 * scale] += 1
    assert int((count == 0).sum()) == 0
    res = preds / count
    return res if ori_size is None else res[:, :, :ori_size[0], :ori_size[1]]


class SyntheticCondEncoder(torch.nn.Module):
    """Parameter-free stand-in for the condition backbone's OUTPUT SHAPES (f, 2f, 4f, 8f channels at 1/4 ... 1/32): average-pooled
    copies of the condition image tiled across channels.  For smoke runs and throughput measurement only."""

    def __init__(self, f=128):
        super().__init__()
        self.f = f

    def forward(self, x):
        feats = []
        for i in range(4):
            p = torch.nn.functional.avg_pool2d(x.float(), 4 << i) if min(x.shape[-2:]) >= (4 << i) else x.float().mean((2, 3), keepdim=True)
            c = self.f << i
            feats.append(p.repeat(1, (c + p.shape[1] - 1) // p.shape[1], 1, 1)[:, :c].contiguous())
        return feats


def resolve_encoder(spec, f=128):
    if spec in (None, "", "none"):
        return None
    if spec == "synthetic":
        return SyntheticCondEncoder(f)
    if spec == "swin_b":
        from adm_amd.unet.swin_transformer import swin_b
        return swin_b()
    mod, attr = spec.split(":")
    obj = getattr(importlib.import_module(mod), attr)
    return obj() if isinstance(obj, type) else obj


class CondStream:
    """Condition / target pairs.  ``data.class_name: synthetic`` draws U(-1,1) high-resolution images and box-downsamples them 4x
    for the condition (the geometry of ddm.data.SRDatasetTest: 'image', 'cond', 'ori_size', 'img_name'); ``data.npy`` may hold
    uint8 [N,H,W,3] high-resolution images.  ``data.class_name: ddm.data.SRDatasetTest`` (+ ``data.npy`` or ``img_folder``) makes the
    condition the reference's test set makes (ddm/data.py:703-722): the image padded with black to multiples of
    256, resized by ``down`` with PIL's bicubic arithmetic on the kernel that makes the training batches (adm_amd.ddm.sr_data), so a
    model sees the same condition at sampling time as in training; 'image' is the unpadded image, as there.  Anything else
    raises (no silent noise for a config that names a real dataset)."""

    def __init__(self, data_cfg, n, device, seed):
        import numpy as np
        self.n, self.device = n, device
        self.gen = torch.Generator(device=device).manual_seed(seed)
        self.images = None
        self.size = tuple(data_cfg.get("image_size") or (512, 512))
        path, cls = data_cfg.get("npy"), data_cfg.get("class_name")
        self.u8, self.names = None, None
        self.down, self.filter = int(data_cfg.get("down") or 4), data_cfg.get("inter_type") or "bicubic"
        if cls in ("ddm.data.SRDatasetTest", "SRDatasetTest"):
            if self.down != 4:
                raise NotImplementedError("the sliding-window sampler places its windows at x4 (reference :324-328): data.down must be 4")
            if path:
                if not os.path.exists(path):
                    raise FileNotFoundError(f"data.npy: {path} does not exist")
                arr = np.load(path, allow_pickle=False)
                if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[-1] != 3:
                    raise ValueError(f"image array must be uint8 [N,H,W,3], got {arr.dtype} {arr.shape}")
                self.u8, self.names = list(arr), [f"{i: 010d}.png" for i in range(arr.shape[0])]
            elif data_cfg.get("img_folder"):
                from adm_amd.ddm.sr_data import load_image_folder
                self.u8, self.names = load_image_folder(data_cfg.get("img_folder"))
            else:
                raise ValueError("data.class_name ddm.data.SRDatasetTest needs data.npy or data.img_folder")
        elif path:
            if not os.path.exists(path):
                raise FileNotFoundError(f"data.npy: {path} does not exist")
            arr = np.load(path, allow_pickle=False)
            if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[-1] != 3:
                raise ValueError(f"image array must be uint8 [N,H,W,3], got {arr.dtype} {arr.shape}")
            self.images = torch.from_numpy(arr).permute(0, 3, 1, 2).float() / 127.5 - 1.0
        elif cls != "synthetic":
            raise NotImplementedError(f"data.class_name {cls!r}: only a uint8 data.npy or 'synthetic' are implemented")

    def sr_test_item(self, i):
        """SRDatasetTest.__getitem__ (data.py:703-722) for image i."""
        import numpy as np
        from adm_amd.ddm.sr_data import resample_image
        img = self.u8[i % len(self.u8)]
        H, W = img.shape[:2]
        pad = np.zeros((-(-H // 256) * 256, -(-W // 256) * 256, 3), dtype=np.uint8)
        pad[:H, :W] = img
        image, cond, _ = resample_image(pad, self.down, self.filter, self.device)
        return {"image": image[:, :, :H, :W].contiguous(), "cond": cond, "ori_size": (H, W), "img_name": self.names[i % len(self.u8)]}

    def __iter__(self):
        for i in range(self.n):
            if self.u8 is not None:
                yield self.sr_test_item(i)
                continue
            if self.images is not None:
                img = self.images[i % self.images.shape[0]][None].to(self.device)
            else:
                img = torch.rand(1, 3, *self.size, device=self.device, generator=self.gen) * 2 - 1
            H, W = img.shape[-2:]
            Hp, Wp = (H + 3) // 4 * 4, (W + 3) // 4 * 4
            pad = torch.nn.functional.pad(img, (0, Wp - W, 0, Hp - H), mode="replicate")
            yield {"image": pad, "cond": torch.nn.functional.avg_pool2d(pad, 4), "ori_size": (H, W), "img_name": f"{i: 010d}.png"}


class DatasetCondStream:
    """The test items of an entry of adm_amd.ddm.datasets.DATASETS that has a ``sampling`` column (in-painting, saliency,
    sketch-to-image), keyed as CondStream's: image or pair i of the pool in order, made one at a time by the kernel that makes the
    training batches (``cond_stream`` with injected draws), never flipped.  The entry says whether ``split: test`` is required,
    and how 'ori_size' and 'img_name' read (``item``); an item without a file name is numbered."""

    def __init__(self, entry, data_cfg, n, image_size, device, seed, want_u8=False):
        """`want_u8`: the items also carry the planes' bytes ('image_u8', 'cond_u8'); asked for by a saliency-scoring run only."""
        sm = entry.sampling
        if sm.split_test and (data_cfg.get("split") or "train") != "test":
            raise ValueError(sm.split_test)
        if sm.no_flip:          # the reference's test transform has no flip (ddm/data.py:377-379)
            data_cfg = dict(data_cfg, augment_horizontal_flip=False)
        self.n, self.item = n, sm.item
        self.extra = {"want_u8": True} if want_u8 else {}
        self.stream = entry.cond_stream(data_cfg, 1, image_size, device, seed)

    def __iter__(self):
        s = self.stream
        for i in range(self.n):
            k = i % s.pool.n
            batch = s.next_batch(idx=[k], flip=[0], **self.extra)
            batch["ori_size"], name = self.item(s, k, batch)
            batch["img_name"] = name or f"{i: 010d}.png"
            yield batch


def start(description):
    """The conditional samplers' preamble: (args, cfg, world, rank, device) of the command line, YAML and launcher; seed 42 + rank."""
    ap = argparse.ArgumentParser(description=description)
    ap.add_argument("--cfg", required=True)
    ap.add_argument("--max-images", type=int, default=None)
    ap.add_argument("--random-init", action="store_true", help="smoke runs: sample without loading a checkpoint")
    args = ap.parse_args()
    with open(args.cfg) as f:
        cfg = Cfg(yaml.load(f, Loader=yaml.SafeLoader))
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.manual_seed(42 + rank)
    return args, cfg, world, rank, device


def load_checkpoint(model, s, random_init, device, lost_message, check=True):
    """Loads ``sampler.ckpt_path`` (EMA weights when ``sampler.use_ema``) unless `random_init`; with `check`, a checkpoint that lacks
    tensors of the condition encoder is refused with `lost_message` (formatted with path, n, first)."""
    if s.get("ckpt_path") and not random_init:
        if not os.path.exists(s.ckpt_path):
            raise FileNotFoundError(f"sampler.ckpt_path {s.ckpt_path} does not exist (pass --random-init for a smoke run)")
        missing, _ = load_weights(model, s.ckpt_path, s.get("use_ema", True), device)
        # (norm.* / head.* of the encoder are holders its forward never reads; an EMA copy holds trained tensors only, so lacks them)
        lost = [k for k in missing if ".init_conv_mask." in k and ".init_conv_mask.norm." not in k and ".init_conv_mask.head." not in k]
        if check and lost:
            raise RuntimeError(lost_message.format(path=s.ckpt_path, n=len(lost), first=lost[0]))
    elif not random_init:
        raise ValueError("sampler.ckpt_path is empty (pass --random-init for a smoke run)")


def save_prediction(img, folder, img_name, world, index, gray=False):
    """img [C,H,W] in [0,1] as an 8-bit png (mode L for one channel when `gray`) under the item's own name, or -- several ranks --
    under its global index; returns the file name."""
    from PIL import Image
    arr = (img.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    name = img_name if world == 1 else f"{index: 010d}.png"
    Image.fromarray(arr[:, :, 0] if gray and arr.shape[2] == 1 else arr).save(os.path.join(folder, name))
    return name


def save_depth_prediction(img, folder, img_name, world, index):
    """img [1,H,W] depth fraction as a 16-bit png (mode I;16) of round(clip(p, 0, 1) * 10000) raw units -- millimetres, as the
    dataset's own depth files -- under the item's own name, or -- several ranks -- under its global index; returns the file name."""
    import numpy as np
    from adm_amd.ddm.depth_data import DEPTH_UNITS, write_depth_png
    units = (img[0].to(torch.float32).clamp(0, 1) * DEPTH_UNITS).round().to(torch.int32).cpu().numpy().astype(np.uint16)
    name = img_name if world == 1 else f"{index: 010d}.png"
    write_depth_png(os.path.join(folder, name), units)
    return name


def saliency_scorer(data_cfg, s):
    """The SaliencyScore of ``sampler.cal_saliency: True`` (``sampler.saliency_normalize``, default True), or None without the key.
    The key on a data set whose ``sampling`` entry is not a saliency one raises."""
    if not bool(s.get("cal_saliency", False)):
        return None
    key = sampling_dataset(data_cfg)
    if key is None or not DATASETS[key].sampling.saliency:
        raise ValueError(f"sampler.cal_saliency: True scores saliency maps, but data.class_name {(data_cfg or {}).get('class_name')!r} "
                         "has none: only ddm.data.DUTSDataset is scored (drop the key)")
    from adm_amd.metrics.saliency import SaliencyScore
    return SaliencyScore(bool(s.get("saliency_normalize", True)))


def report_saliency(score, out_dir, world, rank):
    """Prints the eight values and writes <out_dir>/saliency_metrics.json (several ranks: saliency_metrics_rank{r}.json)."""
    import json
    from adm_amd.metrics.saliency import KEYS
    res = score.result()
    print(f"rank {rank}: saliency score over {res['images']} images: " + " ".join(f"{k}={res[k]:.4f}" for k in KEYS))
    with open(os.path.join(out_dir, "saliency_metrics.json" if world == 1 else f"saliency_metrics_rank{rank}.json"), "w") as f:
        json.dump(res, f)
    return res


def restoration_scorer(data_cfg, s):
    """The RestorationScore of ``sampler.cal_restoration: True`` (``sampler.restoration_crop_border``: default 4 for the x4
    super-resolution form, else 0), or None without the key.  Scored are the entries that print a PSNR and write colour: the
    super-resolution fall-through and in-painting; the key on any other data set raises."""
    if not bool(s.get("cal_restoration", False)):
        return None
    key = sampling_dataset(data_cfg)
    sm = SR_SAMPLING if key is None else DATASETS[key].sampling
    if not sm.psnr or sm.gray:
        raise ValueError(f"sampler.cal_restoration: True scores restored photographs, but data.class_name "
                         f"{(data_cfg or {}).get('class_name')!r} has none: only super-resolution (ddm.data.SRDatasetTest, synthetic) and "
                         "ddm.data.InpaintDataset are scored (drop the key)")
    from adm_amd.metrics.restoration import RestorationScore
    border = s.get("restoration_crop_border")
    return RestorationScore((4 if sm.form == "slide_x4" else 0) if border is None else int(border))


def report_restoration(score, out_dir, world, rank):
    """Prints the values and writes <out_dir>/restoration_metrics.json (several ranks: restoration_metrics_rank{r}.json)."""
    import json
    res = score.result()
    print(f"rank {rank}: restoration score over {res['images']} images (crop_border {score.crop_border}): "
          + " ".join(f"{k}={res[k]:.4f}" for k in res if k != "images"))
    with open(os.path.join(out_dir, "restoration_metrics.json" if world == 1 else f"restoration_metrics_rank{rank}.json"), "w") as f:
        json.dump(res, f)
    return res


def window_sampler(ldm, scale):
    """c [B,C,h,w] -> the sample for the window c, `scale` times its size.  The encoder runs ONCE per window batch (the reference
    re-runs it inside every denoising step, cond_unet_sd.py:821)."""
    down = ldm.first_stage_model.down_ratio
    return lambda c: ldm.sample(cond=list(ldm.model.init_conv_mask(c)), latent_hw=(c.shape[2] * scale // down, c.shape[3] * scale // down))


def predict_composite(ldm, s, batch, crop, stride):
    """In-painting: kept pixels from the masked image, holes from the sample (reference :175-186, ddm_const_2.py:629)."""
    cond = batch["cond"]
    return ldm.sample(cond=list(ldm.model.init_conv_mask(cond)), mask=batch["ori_mask"], cond_image=cond).to(torch.float32)


def predict_window(ldm, s, batch, crop, stride):
    """Sketch-to-image: one window, the whole one-channel condition."""
    cond = batch["cond"]
    if cond.shape[1] != 1 or int(s.get("out_channels", 3)) != 3:
        raise ValueError(f"sketch-to-image takes a one-channel condition and makes three channels, got cond {tuple(cond.shape)}, "
                         f"sampler.out_channels {s.get('out_channels', 3)}")
    return window_sampler(ldm, 1)(cond).to(torch.float32)


def predict_slide(ldm, s, batch, crop, stride, scale=1, out_channels=1, ori_size=None):
    """Saliency: the reference's slide_sample (:220-283), windows over the condition at the output's own resolution.  With scale 4,
    three channels and the item's ``ori_size``: super-resolution -- the frame the windows tile is the condition's, x4 (for
    SRDatasetTest larger than the unpadded image: reference :324-332)."""
    cond = batch["cond"]
    return slide_sample_sr(window_sampler(ldm, scale), cond, (cond.shape[-2] * scale, cond.shape[-1] * scale), crop, stride,
                           out_channels=int(s.get("out_channels", out_channels)), scale=scale, ori_size=ori_size,
                           window_batch=int(s.get("window_batch", 0)), flip_test=bool(s.get("flip_test", False)))


# Sampling.form of adm_amd.ddm.datasets -> (ldm, sampler cfg, item, crop, stride) -> the prediction [1,C,H,W] in [0,1]
FORMS = {"composite": predict_composite, "window": predict_window, "slide": predict_slide,
         "slide_x4": lambda ldm, s, batch, crop, stride: predict_slide(ldm, s, batch, crop, stride, 4, 3, batch["ori_size"])}


def main():
    args, cfg, world, rank, device = start("sliding-window conditional latent sampler (MI355X hot path)")
    mc, s = cfg.model, cfg.sampler
    assert mc.get("ldm"), "this driver is for latent models (reference :58)"
    ldm = build_model(mc).to(device).eval()
    builtin = s.get("cond_encoder") == "swin_b"
    enc = getattr(ldm.model, "init_conv_mask", None) if builtin else None          # (unet.cond_encoder: swin_b built it already)
    if not builtin and isinstance(getattr(ldm.model, "init_conv_mask", None), torch.nn.Module):
        raise ValueError(f"the unet section built its own condition encoder (cond_encoder: swin_b) but sampler.cond_encoder is "
                         f"{s.get('cond_encoder')!r}: set sampler.cond_encoder: swin_b, or drop the key from the unet section")
    if enc is None:
        enc = resolve_encoder(s.get("cond_encoder"), getattr(ldm.model, "f_cond", 128))
    if enc is None:
        raise ValueError("sampler.cond_encoder is required: 'swin_b' (the built-in encoder, weights from the checkpoint), "
                         "'module:callable' returning the four condition feature maps, or 'synthetic'")
    ldm.model.init_conv_mask = enc.to(device) if isinstance(enc, torch.nn.Module) else enc
    load_checkpoint(ldm, s, args.random_init, device, "sampler.cond_encoder: swin_b, but {path} lacks {n} of the encoder's tensors "
                    "(first: {first}): the checkpoint must hold the trained init_conv_mask.* weights", check=builtin)
    out_dir = s.save_folder
    os.makedirs(out_dir, exist_ok=True)
    n_total = int(s.sample_num) if args.max_images is None else min(int(s.sample_num), args.max_images)
    per_rank = n_total // world
    key = sampling_dataset(cfg.data)
    saliency_score = saliency_scorer(cfg.data, s)
    restoration_score = restoration_scorer(cfg.data, s)
    if key is None:
        sm = SR_SAMPLING
        stream = CondStream(cfg.data, per_rank, device, seed=2000 + rank)
        crop, stride = tuple(s.crop_size), tuple(s.stride)
    else:
        sm = DATASETS[key].sampling
        size = tuple(cfg.data.get("image_size") or mc.image_size)
        stream = DatasetCondStream(DATASETS[key], cfg.data, per_rank, size, device, seed=2000 + rank, want_u8=saliency_score is not None)
        # The reference's in-painting and saliency sample YAMLs have neither key, and its own driver would fail on them
        # (cfg.sampler.crop_size, :190): they default to one window, the image at model resolution.
        crop = tuple(s.get("crop_size") or size)
        stride = None if sm.form == "window" else tuple(s.get("stride") or size)
        if sm.one_window and crop != size:
            raise NotImplementedError(f"{sm.one_window} samples the whole image in one window: sampler.crop_size {crop} must equal image_size {size}")
    masks = sm.save_masks and bool(s.get("save_masks", False))
    if masks:
        os.makedirs(os.path.join(out_dir, "masks"), exist_ok=True)
    depth_score = None
    if sm.depth:
        from adm_amd.metrics.depth import KEYS, DepthScore
        depth_score = DepthScore(float(s.get("min_depth", 1e-3)), float(s.get("max_depth", 10.0)))
    psnr, done, t0 = 0.0, 0, time.time()
    for batch in stream:
        pred = FORMS[sm.form](ldm, s, batch, crop, stride)
        if sm.psnr:          # (reference :195) against the part of 'image' the prediction covers: SRDatasetTest cuts it to ori_size
            image = (batch["image"] + 1) * 0.5
            psnr += float(-10.0 * torch.log10(torch.mean((pred - image[:, :, :pred.shape[2], :pred.shape[3]]) ** 2)))
        if depth_score is not None:          # on the device; the sums are copied to the host once, at the end
            depth_score.add(pred.to(torch.float32).contiguous(), ((batch["image"] + 1) * 0.5).contiguous())
        if saliency_score is not None:          # the bytes the png below holds against the resized map's bytes; tables stay on the device
            saliency_score.add(pred[:, :1].to(torch.float32).contiguous(), batch["image_u8"])
        if restoration_score is not None:          # the bytes the png below holds against the target's; the sums stay on the device
            target = (batch["image"] + 1) * 0.5
            restoration_score.add(pred.to(torch.float32).contiguous(), target[:, :, :pred.shape[2], :pred.shape[3]].to(torch.float32).contiguous())
        if sm.depth and not bool(s.get("depth_png8", False)):
            name = save_depth_prediction(pred[0], out_dir, batch["img_name"], world, rank * per_rank + done)
        else:
            name = save_prediction(pred[0], out_dir, batch["img_name"], world, rank * per_rank + done, sm.gray)
        if masks:
            save_prediction(batch["ori_mask"][0], os.path.join(out_dir, "masks"), name, 1, 0, gray=True)          # 0 / 1 -> 0 / 255
        done += 1
    torch.cuda.synchronize()
    dt = time.time() - t0
    score = f"; PSNR: {psnr / max(done, 1):.2f}" if sm.psnr else ""
    print(f"rank {rank}: {done} images in {dt:.1f}s ({done / max(dt, 1e-9):.2f} images/sec incl. PNG writes){score}")
    if depth_score is not None:
        import json
        res = depth_score.result()
        print(f"rank {rank}: depth score over {res['images']} images ({res['skipped']} without a valid pixel): "
              + " ".join(f"{k}={res[k]:.4f}" for k in KEYS))
        with open(os.path.join(out_dir, "depth_metrics.json" if world == 1 else f"depth_metrics_rank{rank}.json"), "w") as f:
            json.dump(res, f)
    if saliency_score is not None:
        report_saliency(saliency_score, out_dir, world, rank)
    if restoration_score is not None:
        report_restoration(restoration_score, out_dir, world, rank)


if __name__ == "__main__":
    main()
