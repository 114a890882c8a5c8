#!/usr/bin/env python3
"""MI355X counterpart of the reference's first-stage trainer (train_vae.py): trains the KL autoencoder with the
LPIPS + PatchGAN loss on the HIP hot path.

Same command line and YAML schema (``--cfg <yaml>`` with sections model{class_name, embed_dim, lossconfig, ddconfig, ckpt_path},
data, trainer); the recipe it reproduces:
  two optimisers    AdamW(lr) over encoder + decoder + quant_conv + post_quant_conv, AdamW(lr) over loss.discriminator;
                    loss.logvar is in neither (as in the reference, where it keeps its initial value)
  schedule          lr * max((1 - it / N) ** 0.95, min_lr / lr) for both
  micro-steps       the micro-step index doubles as optimizer_idx: with gradient_accumulate_every: 2, micro-step 0 updates the
                    autoencoder and micro-step 1 the discriminator, on the same batch; each loss is divided by the count
  no clipping       the reference's clip_grad_norm_ runs after both optimiser steps and so clips nothing
  EMA               beta 0.995, update_every 10, update_after_step 1000 (trainer.ema_update_after_step), power 2/3, over every
                    parameter and buffer of the model
  checkpoints       {'step', 'model', 'opt_ae', 'lr_scheduler_ae', 'opt_disc', 'lr_scheduler_disc', 'ema', 'scaler'} in
                    ``results_folder/model-{milestone}.pt``; the file loads as a first stage through
                    AutoencoderKL.init_from_ckpt ('ema' and 'model' layouts)

What differs: single process (data-parallel first-stage training is not implemented); the optimisers are torch.optim.AdamW on
ordinary parameters, not the fused flat-buffer optimiser; AutoencoderKL.training_step runs its own backward (see
adm_amd/ddm/loss.py), so the loop calls no .backward().  Data comes from ``first_stage_stream``: the recipe's own dataset
(``ddm.data.ImageDataset``, the maps of ``ddm.data.DUTSDataset``, the photos of ``ddm.data.SketchDataset``, the HR crops of
``ddm.data.SRDataset``, the depth planes of ``ddm.data.NYUDv2DepthDataset``; three or ONE channel), or train_uncond_dpm.ImageStream: ``data.npy`` (uint8 [N,H,W,3]) or
``data.class_name: synthetic``.  LPIPS weights are not shipped: ``model.lossconfig.lpips_ckpt`` or a checkpoint
with ``loss.perceptual_loss.*`` keys provides them; without them the perceptual term is zero (a warning says so).
"""
import argparse
import os
import sys
import time

import torch
import yaml

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from adm_amd.ddm.utils import construct_class_by_name  # noqa: E402
from adm_amd.optim import ema_decay_at  # noqa: E402
from train_uncond_dpm import Cfg, ImageStream, save_grid  # noqa: E402


def vae_lr_lambda(it: int, lr: float, min_lr: float, train_num_steps: int) -> float:
    """The LambdaLR factor of the reference's first-stage Trainer."""
    return max((1 - it / train_num_steps) ** 0.95, min_lr / lr)


def micro_steps(gradient_accumulate_every: int):
    """[(optimizer_idx, optimiser name)] of one step: the micro-step index IS the optimizer index."""
    if gradient_accumulate_every not in (1, 2):
        raise ValueError("gradient_accumulate_every must be 1 (autoencoder only) or 2 (autoencoder, then discriminator): the "
                         "micro-step index is the optimizer index, and there are two optimisers")
    return [(0, "opt_ae"), (1, "opt_disc")][:gradient_accumulate_every]


def ema_action(ema_step: int, initted: bool, update_every: int = 10, update_after_step: int = 1000, beta: float = 0.995):
    """What EMA.update does at its call number `ema_step`: (decay or None for no update, initted afterwards); decay 0.0 = copy."""
    if ema_step % update_every:
        return None, initted
    if ema_step <= update_after_step:
        return 0.0, initted
    if not initted:          # the first update after the warm-up copies, then averages: the copy makes the average a no-op
        return 0.0, True
    return ema_decay_at(ema_step + 1, beta=beta, update_after_step=update_after_step), True


def first_stage_stream(data_cfg, batch, size, device, seed):
    """The batch source of a first stage, by ``data.class_name`` (or ``synthetic_of`` under ``class_name: synthetic``): the
    ``first_stage`` column of adm_amd.ddm.datasets.DATASETS.  ``ddm.data.ImageDataset`` / ``ddm.data.DUTSDataset`` (its maps, one
    channel) / ``ddm.data.SketchDataset`` (its photos) select the one-plane streams of adm_amd/ddm/image_data.py;
    ``ddm.data.NYUDv2DepthDataset`` selects the one-channel ``DepthMapStream`` of adm_amd/ddm/depth_data.py;
    ``ddm.data.SRDataset`` selects ``SRBatchStream``, whose ``image`` -- the HR crop -- is what the DIV2K first stage trains on
    (data.py:645-658); everything else goes to ``ImageStream``, which refuses what it does not build.  The stream carries ``channels``."""
    from adm_amd.ddm.datasets import DATASETS, dataset_of
    from adm_amd.ddm.image_data import ImageBatchStream
    data_cfg = data_cfg or {}
    key = dataset_of(data_cfg)
    picked = DATASETS[key].first_stage if key else None
    if picked is None and data_cfg.get("class_name") == "synthetic" and data_cfg.get("synthetic_of") is not None:
        raise NotImplementedError(f"data.synthetic_of {data_cfg.get('synthetic_of')!r}: a synthetic first-stage pool is built for "
                                  "ddm.data.ImageDataset, ddm.data.DUTSDataset, ddm.data.SketchDataset and ddm.data.SRDataset")
    stream = (picked or ImageStream)(data_cfg, batch, size, device, seed)
    if not isinstance(stream, ImageBatchStream) and not hasattr(stream, "channels"):          # (the one-plane streams say their own)
        stream.channels = 3
    return stream


def check_channels(stream_channels: int, model_cfg):
    """Start-up checks: the stream's channel count against ``ddconfig.in_channels``, and ``lossconfig.disc_in_channels`` against
    ``ddconfig.out_ch`` (the discriminator sees the reconstruction)."""
    dd, lc = model_cfg.get("ddconfig") or {}, model_cfg.get("lossconfig") or {}
    in_ch, out_ch, disc = int(dd.get("in_channels", 3)), int(dd.get("out_ch", 3)), int(lc.get("disc_in_channels", 3))
    if int(stream_channels) != in_ch:
        raise ValueError(f"the data stream yields {int(stream_channels)}-channel images but model.ddconfig.in_channels is {in_ch}")
    if disc != out_ch:
        raise ValueError(f"model.lossconfig.disc_in_channels is {disc} but model.ddconfig.out_ch is {out_ch}: the discriminator "
                         "judges the reconstruction")


def parse_args():
    ap = argparse.ArgumentParser(description="training the KL autoencoder (MI355X hot path)")
    ap.add_argument("--cfg", type=str, required=True)
    ap.add_argument("--max-steps", type=int, default=None, help="stop early (smoke runs)")
    ap.add_argument("--resume", type=int, default=None, help="milestone to resume from (overrides trainer.resume_milestone)")
    args = ap.parse_args()
    with open(args.cfg) as f:
        args.cfg = yaml.load(f, Loader=yaml.SafeLoader)
    return args


class Trainer:
    def __init__(self, model, stream, cfg, device, resume=None):
        t = cfg.trainer
        self.model, self.stream, self.cfg, self.device = model, stream, cfg, device
        self.accum = int(t.get("gradient_accumulate_every", 2))
        self.plan = micro_steps(self.accum)
        self.lr, self.min_lr = float(t.lr), float(t.get("min_lr", 0.0))
        self.train_num_steps = int(t.train_num_steps)
        self.save_every = int(t.get("save_and_sample_every", 5000))
        self.log_freq = int(t.get("log_freq", 200))
        self.ema_beta, self.ema_every = float(t.get("ema_decay", 0.995)), int(t.get("ema_update_every", 10))
        self.ema_after = int(t.get("ema_update_after_step", 1000))
        self.results = t.results_folder
        ae_params = (list(model.encoder.parameters()) + list(model.decoder.parameters()) + list(model.quant_conv.parameters())
                     + list(model.post_quant_conv.parameters()))
        self.opt_ae = torch.optim.AdamW(ae_params, lr=self.lr)
        self.opt_disc = torch.optim.AdamW(model.loss.discriminator.parameters(), lr=self.lr)
        lam = lambda it: vae_lr_lambda(it, self.lr, self.min_lr, self.train_num_steps)      # noqa: E731
        self.lr_scheduler_ae = torch.optim.lr_scheduler.LambdaLR(self.opt_ae, lr_lambda=lam)
        self.lr_scheduler_disc = torch.optim.lr_scheduler.LambdaLR(self.opt_disc, lr_lambda=lam)
        self.step, self.ema_step, self.ema_initted = 0, 0, False
        self.ema = {k: v.detach().clone() for k, v in model.state_dict().items()}
        self.logs = []
        os.makedirs(self.results, exist_ok=True)
        milestone = resume if resume is not None else t.get("resume_milestone", 0)
        if milestone and os.path.exists(os.path.join(self.results, f"model-{milestone}.pt")):
            self.load(milestone)

    # ---- EMA over parameters and buffers, the reference's settings -----------------------------------
    @torch.no_grad()
    def ema_update(self):
        decay, self.ema_initted = ema_action(self.ema_step, self.ema_initted, self.ema_every, self.ema_after, self.ema_beta)
        self.ema_step += 1
        if decay is None:
            return
        for k, v in self.model.state_dict().items():
            e = self.ema.get(k)
            if e is None or e.shape != v.shape:          # (a perceptual network installed after construction)
                self.ema[k] = v.detach().clone()
            elif decay == 0.0 or not v.is_floating_point():
                e.copy_(v)
            else:
                e.lerp_(v, 1.0 - decay)

    def ema_state_dict(self):
        sd = {"ema_model." + k: v.clone() for k, v in self.ema.items()}
        sd["initted"] = torch.tensor([self.ema_initted])
        sd["step"] = torch.tensor([self.ema_step])
        return sd

    # ---- checkpoint layout of the reference's Trainer.save / load --------------------------------------
    def save(self, milestone):
        data = {"step": self.step, "model": self.model.state_dict(), "opt_ae": self.opt_ae.state_dict(),
                "lr_scheduler_ae": self.lr_scheduler_ae.state_dict(), "opt_disc": self.opt_disc.state_dict(),
                "lr_scheduler_disc": self.lr_scheduler_disc.state_dict(), "ema": self.ema_state_dict(), "scaler": None}
        torch.save(data, os.path.join(self.results, f"model-{milestone}.pt"))

    def load(self, milestone):
        data = torch.load(os.path.join(self.results, f"model-{milestone}.pt"), map_location=self.device, weights_only=True)
        self.model.load_state_dict(data["model"])
        self.step = data["step"]
        self.opt_ae.load_state_dict(data["opt_ae"])
        self.opt_disc.load_state_dict(data["opt_disc"])
        self.lr_scheduler_ae.load_state_dict(data["lr_scheduler_ae"])
        self.lr_scheduler_disc.load_state_dict(data["lr_scheduler_disc"])
        for k, v in data["ema"].items():
            if k.startswith("ema_model.") and k[10:] in self.ema:
                self.ema[k[10:]].copy_(v)
        self.ema_step = int(data["ema"].get("step", torch.tensor([0]))[0])
        self.ema_initted = bool(data["ema"].get("initted", torch.tensor([False]))[0])
        from adm_amd import ops
        ops.invalidate_packed()

    def train(self, max_steps=None):
        last, seen = time.time(), 0
        end = self.train_num_steps if max_steps is None else min(self.train_num_steps, self.step + max_steps)
        while self.step < end:
            img = next(self.stream)["image"]
            log = {}
            for idx, name in self.plan:
                if idx == 0:
                    self.opt_ae.zero_grad(set_to_none=True)
                    self.opt_disc.zero_grad(set_to_none=True)
                else:
                    self.opt_disc.zero_grad(set_to_none=True)
                _, lg = self.model.training_step(img, idx, self.step, loss_scale=1.0 / self.accum)
                getattr(self, name).step()
                log.update(lg)
            self.lr_scheduler_ae.step()
            self.lr_scheduler_disc.step()
            seen += img.shape[0]
            wanted = self.step % self.log_freq == 0 or self.step + 1 == end
            self.step += 1
            self.ema_update()
            if wanted:       # the only host copies of the loop: the log's device scalars, when a line is printed
                vals = {k.split("/", 1)[-1]: float(v) for k, v in log.items()}
                self.logs.append((self.step - 1, vals))
                dt = time.time() - last
                print(f"[Train Step] {self.step - 1}/{self.train_num_steps}: " + " ".join(f"{k}={v:.6g}" for k, v in vals.items())
                      + f" lr={self.opt_ae.param_groups[0]['lr']:.3e} images/sec={seen / dt:.1f}", flush=True)
                last, seen = time.time(), 0
            if self.step % self.save_every == 0:
                milestone = self.step // self.save_every
                self.save(milestone)
                self.model.eval()
                with torch.no_grad():
                    rec, _ = self.model(img[:2])
                self.model.train()
                save_grid((rec + 1.0) / 2.0, os.path.join(self.results, f"sample-{milestone}.png"), 2)
        print("training complete")


def main(args):
    cfg = Cfg(args.cfg)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("train_vae.py is single-process: data-parallel first-stage training is not implemented")
    local = int(os.environ.get("ADM_LOCAL_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    size = tuple(cfg.data.get("image_size") or cfg.model.ddconfig.resolution)
    stream = first_stage_stream(cfg.data, int(cfg.data.batch_size), size, device, seed=1000)
    check_channels(stream.channels, cfg.model)
    model = construct_class_by_name(**{k: v for k, v in cfg.model.items()}).to(device)
    model.enable_training()
    model.train()
    trainer = Trainer(model, stream, cfg, device, resume=args.resume)
    trainer.train(args.max_steps)


if __name__ == "__main__":
    main(parse_args())
