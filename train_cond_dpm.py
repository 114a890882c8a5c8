#!/usr/bin/env python3
"""MI355X counterpart of the reference's conditional PIXEL-SPACE trainer (its train_cond_dpm.py): the saliency recipe without a
first stage (configs/saliency/duts_cond_ddm_const_dpm.yaml; reference configs/saliency/DUTS_ddm_const_dpm_114.yaml) --
ddm.ddm_const.DDPM with use_l1, weighting_loss and the LPIPS term on the one-channel map, unet.cond_unet.Unet at channels 1 and the
Swin-B condition encoder trained along.

Same command line (``--cfg``, ``--max-steps``) and YAML schema as the other drivers.  Model construction [:40-48], gradient
accumulation [:253-282], clip-norm [:294], EMA [:189-191, 311-312], the checkpoint layout [:209-222] and the multi-GPU launch are
the shared Trainer of train_uncond_dpm.py, through the CondTrainer of train_cond_ldm.py.  What the reference's train_cond_dpm.py
does differently from its unconditional driver, and this one with it (reference lines in brackets):
  * batch source: {'image': map [B,1,H,W], 'cond': photo [B,3,H,W]} of ddm.data.DUTSDataset [:50-51, :88-89], made on the device by
    adm_amd.ddm.pair_data.DUTSBatchStream; ``class_name: synthetic`` + ``synthetic_of: ddm.data.DUTSDataset`` runs without data;
  * training_step passes batch['cond'] to the denoiser (ddm_const_2.py:157-161) [:267-269];
  * LR schedule: ratio max((1 - it/N)^0.96, min_lr/lr) from step 0, no warm-up [:183];
  * weight decay defaults to 1e-2 [:98];
  * the ``test_before`` sample is conditioned on a training batch, sample(batch_size=cond.shape[0], cond=cond) with no mask, written
    as ``sample-{resume_milestone}_{sampling_timesteps}.png`` on 2^floor(log2(sqrt(batch_size))) columns [:100-122];
  * the periodic sample is conditioned on the last training micro-batch [:325-337].
What differs from the reference: the condition encoder runs once per sample() instead of once per sampler step (same bits in eval
mode); batches are always full (the stream has no short last batch); ``sampler.test_in_train`` (FID through an external tool
[:339-373]) is not built.  f32 compute mode only.
"""
import torch

import train_cond_ldm
from train_cond_ldm import CondTrainer, grid_columns
from train_uncond_dpm import parse_args, save_grid


class PixelCondTrainer(CondTrainer):
    def cond_sample(self, batch, path):
        """train_cond_dpm.py:100-122, 325-337: one sample per condition photo of `batch`; the pixel-space sample() has no mask."""
        self.model.eval()
        with torch.no_grad():
            img = self.model.sample(batch_size=batch["cond"].shape[0], cond=batch["cond"])
        self.model.train()
        save_grid(img, path, grid_columns(batch["cond"].shape[0]))


def check_cfg(cfg):
    from adm_amd import ops
    if ops.COMPUTE != "f32":
        raise NotImplementedError("train_cond_dpm.py runs in the f32 compute mode only (the LPIPS term and the Swin encoder's "
                                  "backward are not built for the bf16 mode)")
    model = cfg["model"]
    if model.get("ldm") or model.get("first_stage"):
        raise ValueError("train_cond_dpm.py trains pixel-space models (ldm: False, no first_stage); use train_cond_ldm.py")
    if (cfg.get("sampler") or {}).get("test_in_train"):
        raise NotImplementedError("sampler.test_in_train (FID through an external tool) is not built")


def main(args):
    check_cfg(args.cfg)
    train_cond_ldm.main(args, trainer_cls=PixelCondTrainer)


if __name__ == "__main__":
    main(parse_args())
