#!/usr/bin/env python3
"""MI355X counterpart of the reference's conditional LATENT trainer (its train_cond_ldm.py): the 4x super-resolution
recipe (configs/super-resolution/div2k_cond_ddm_const_ldm_train.yaml), the in-painting recipe
(configs/inpainting/celebahq_cond_ddm_const_ldm.yaml), the saliency recipe (configs/saliency/duts_cond_ddm_const_ldm.yaml), the
sketch-to-image recipe (configs/sketch2img/sketchcoco_cond_ddm_const_ldm.yaml) and the depth recipe
(configs/depth_estimation/nyud_cond_ddm_const_ldm.yaml).

Same command line and YAML schema as the other drivers (``--cfg``, ``--max-steps``); model construction, gradient accumulation,
clip-norm, EMA, the checkpoint layout and the multi-GPU launch are the shared Trainer of train_uncond_dpm.py.  What differs from
that driver (reference lines of train_cond_ldm.py in brackets):
  * batch source: {'image', 'cond'} pairs of ddm.data.SRDataset [:57-63], made on the device by one HIP kernel from a uint8
    image pool (adm_amd.ddm.sr_data.SRBatchStream) instead of PIL in dataloader workers; with ``data.class_name:
    ddm.data.InpaintDataset`` the {'image', 'cond', 'ori_mask'} triples of adm_amd.ddm.inpaint_data.InpaintBatchStream; with
    ``ddm.data.DUTSDataset`` the {'image': map, 'cond': photo} pairs of adm_amd.ddm.pair_data.DUTSBatchStream; with
    ``ddm.data.SketchDataset`` the {'image': photo, 'cond': sketch} pairs of its SketchBatchStream; with
    ``ddm.data.NYUDv2DepthDataset`` the {'image': depth, 'cond': photo} crops of adm_amd.ddm.depth_data.DepthBatchStream;
  * LR schedule: ratio max((1 - it/N)^0.96, min_lr/lr) from step 0, no warm-up [:150];
  * weight decay defaults to 1e-2 [:72];
  * the periodic and ``test_before`` samples are conditioned on a training batch: sample(batch_size=cond.shape[0], cond=..., mask=
    batch.get('ori_mask')) on a grid of 2^floor(log2(sqrt(B))) columns [:80-90, 297-310]; the ``test_before`` file is
    ``sample-{resume_milestone}_{sampling_timesteps}.png`` [:90].
The checkpoint's 'model' (and 'ema') carries ``init_conv_mask.*`` when the unet section builds the condition encoder
(``cond_encoder: swin_b``); with ``train_cond_encoder: True`` its tensors are trained (the Unet is constructed before the flat
parameter buffer).  ``unet.cond_encoder_weights`` starts the encoder from a local ImageNet state dict; nothing is fetched.
"""
import math
import os
import warnings

import torch
import torch.distributed as dist

from train_uncond_dpm import Cfg, Trainer, build_model, parse_args, save_grid
from adm_amd.ddm.datasets import DATASETS, dataset_of
from adm_amd.ddm.sr_data import SRBatchStream
from adm_amd.optim import lr_lambda_cond


def grid_columns(batch):
    return 2 ** math.floor(math.log2(math.sqrt(batch)))          # train_cond_ldm.py:89, 309


def batch_stream(data_cfg, batch, image_size, device, seed):
    """The batch source ``data.class_name`` names (the ``cond_stream`` column of adm_amd.ddm.datasets.DATASETS): in-painting triples
    for ddm.data.InpaintDataset, saliency pairs for ddm.data.DUTSDataset, sketch-to-image pairs for ddm.data.SketchDataset,
    super-resolution pairs otherwise (SRBatchStream raises for what it does not know).  ``class_name: synthetic`` stands for the
    dataset ``data.synthetic_of`` names."""
    key = dataset_of(data_cfg)
    picked = (DATASETS[key].cond_stream if key else None) or SRBatchStream
    return picked(data_cfg, batch, image_size, device, seed)


class CondTrainer(Trainer):
    def __init__(self, model, stream, cfg, device, rank, world):
        if cfg.trainer.get("weight_decay") is None:
            cfg.trainer["weight_decay"] = 1e-2                   # train_cond_ldm.py:72
        super().__init__(model, stream, cfg, device, rank, world)

    def _lr_ratio(self, it):
        return lr_lambda_cond(it, self.lr, self.min_lr, self.train_num_steps)      # train_cond_ldm.py:150

    def cond_sample(self, batch, path):
        """train_cond_ldm.py:297-310: one sample per condition image of `batch`."""
        self.model.eval()
        with torch.no_grad():
            img = self.model.sample(batch_size=batch["cond"].shape[0], cond=batch["cond"], mask=batch.get("ori_mask"))
        self.model.train()
        save_grid(img, path, grid_columns(batch["cond"].shape[0]))

    def sample_grid(self, milestone, batch):
        self.cond_sample(batch, os.path.join(self.results, f"sample-{milestone}.png"))


def main(args, trainer_cls=None):
    cfg = Cfg(args.cfg)
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("ADM_LOCAL_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("ADM_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)
    model_cfg = cfg.model
    unet_cfg = model_cfg.unet
    if unet_cfg.get("train_cond_encoder") and not unet_cfg.get("cond_encoder_weights") and not cfg.trainer.get("resume_milestone"):
        warnings.warn("unet.cond_encoder_weights is not set: the condition encoder starts from its own initialisation; the "
                      "reference starts it from torchvision's ImageNet Swin-B weights (swin_transformer.py:452-459)")
    ldm = build_model(model_cfg).to(device).train()          # the Unet (and its encoder) exists before FlatParams is built
    global_batch = int(cfg.data.batch_size)
    assert global_batch % world == 0, "split_batches: the YAML batch_size is the global batch"
    stream = batch_stream(cfg.data, global_batch // world, tuple(cfg.data.get("image_size") or model_cfg.image_size), device,
                          seed=1000 + rank)
    trainer = (trainer_cls or CondTrainer)(ldm, stream, cfg, device, rank, world)
    if cfg.trainer.get("test_before", False) and rank == 0:          # train_cond_ldm.py:74-91
        name = f"sample-{cfg.trainer.get('resume_milestone', 0)}_{model_cfg.sampling_timesteps}.png"
        trainer.cond_sample(next(stream), os.path.join(cfg.trainer.results_folder, name))
    trainer.train(args.max_steps)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(parse_args())
