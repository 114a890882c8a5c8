"""HIP drop-in for the reference's ddm/ddm_linear.py ``DDPM``: the linear-drift formulation

    U(t) = K t^2 / 2 + C t,   U(1) = -x0  =>  C = -x0 - K / 2,      x_t = x0 + U(t) + sqrt(t) eps.

The denoiser predicts ``theta = [K | C]`` (six channels: ``out_mul: 2`` of the two-decoder UNet, which the reference can only run
with ``precondition: False``) and the noise.  Arithmetic restated from ddm_linear.py: q_sample :168-171, pred_x0 :173-176,
reverse step :178-186, p_losses :188-242, sample_fn :272-310.

What differs from the const wrappers (adm_amd/ddm/ddpm.py), as in the reference:
  * ``K ~ N(0, 1)`` clamped to [-1, 1] is drawn per element after the noise; the sampler clamps the predicted K the same way;
  * the losses use the 'mean' reduction: ``loss_simple = mean_b [w1 mean (theta_pred - [K|C])^2 + w2 mean (noise_pred - eps)^2]``
    (``use_l1`` adds the mean-|.| twins and halves), ``w1 = 1/t``, ``w2 = 1/(1 - t + eps)`` under ``weighting_loss``;
  * ``loss_vlb = mean_b (MAE_b [+ LPIPS_b]) * mean_b (1 - t_b)^2``: the reference multiplies a [B] vector by a [B,1] one and takes
    the mean of the [B,B] result, which is that product.  The MAE part is always on; the LPIPS summand follows the rule of the
    const wrappers (weights supplied -> on, else a warning and no LPIPS summand);
  * the log values are the reference's (no further division);
  * ``sample()`` is the stochastic Euler sampler with ``denoise=True``: ``sampling_timesteps + 1`` network evaluations on an fp32
    state with an fp32 time vector, and returns float32.

Every draw is injectable (``t=``, ``noise=``, ``K=``, ``x_T=``, ``epsilons=``, ``augment_draws=``).  The whole loss (both means,
the MAE term, both gradients) is one launch (``adm_ddm_loss_linear``).  The sampler launches eagerly: ``ADM_SAMPLE_GRAPH`` is not read.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import ops
from .ddpm import DDPMBase, _cfg_get


class DDPM(DDPMBase):
    SCHEDULE = "linear"
    DEFAULT_EPS = 1e-4
    AUGMENT_P = 0.12           # ddm_linear.py:110
    NO_LPIPS_WARNING = ("adm_amd: the LPIPS term (perceptual_weight > 0) needs VGG16 weights that cannot be fetched offline; "
                        "loss_vlb is its MAE part alone (see DESIGN.md)")

    def __init__(self, model, *, image_size, sample_type="naive", **kwargs):
        cfg = kwargs.get("cfg", None)
        st = _cfg_get(cfg, "sample_type", "euler")
        if st != "euler":        # the reference's sample() would call sample_fn_2order, which does not exist
            raise NotImplementedError(f"sample_type {st!r}: the linear-drift DDM has the 'euler' sampler only")
        super().__init__(model, image_size=image_size, sample_type=sample_type, **kwargs)
        if ops.COMPUTE != "f32":
            raise NotImplementedError("the linear-drift DDM runs in the f32 compute mode only")
        out_mul = getattr(getattr(self.model, "model", None), "out_mul", 2)
        if out_mul != 2:
            raise ValueError(f"ddm_linear.DDPM needs a denoiser with out_mul: 2 (theta = [K | C]), got out_mul = {out_mul}")

    # ------------------------------------------------------------------ schedule pieces
    @staticmethod
    def _bc(t, like):
        return t.reshape(like.shape[0], *((1,) * (like.dim() - 1)))

    def q_sample(self, x_start, noise, t, K, C=None):
        """x_t = x0 + K t^2/2 + C t + sqrt(t) eps.  With C = -x0 - K/2 (None: the only C the wrapper uses) one HIP launch that also
        clamps K to [-1, 1]; any other C is the API-parity broadcast form."""
        if C is None:
            return ops.q_sample_linear(x_start, noise, K, t.to(torch.float32))
        time = self._bc(t, C)
        return x_start + K / 2 * time ** 2 + C * time + torch.sqrt(time) * noise

    def pred_x0_from_xt(self, xt, noise, t, K, C):
        """x0 = x_t - K t^2/2 - C t - sqrt(t) eps (ddm_linear.py:173-176; the loss and LPIPS-input kernels do this inside)."""
        time = self._bc(t, C)
        return xt - K / 2 * time ** 2 - C * time - torch.sqrt(time) * noise

    def pred_xtms_from_xt(self, xt, noise, K, C, t, s, epsilon=None):
        """One stochastic reverse step (ddm_linear.py:178-186); `epsilon` injectable.  API-parity helper: sample_fn does this in
        its fused step kernel."""
        time, s = self._bc(t, C), self._bc(s, C)
        mean = xt + K / 2 * s ** 2 - K * time * s - C * s - s / torch.sqrt(time) * noise
        if epsilon is None:
            epsilon = torch.randn_like(mean)
        return mean + torch.sqrt(s * (time - s) / time) * epsilon

    def loss_weights(self, t):
        if not self.weighting_loss:
            return torch.ones_like(t), torch.ones_like(t)
        return 1 / t, 1 / (1 - t + self._eps_f)          # ddm_linear.py:213-216

    # ------------------------------------------------------------------ training
    def p_losses(self, x_start, t, *args, noise: Optional[torch.Tensor] = None, K: Optional[torch.Tensor] = None, **kwargs):
        if noise is None:
            noise = torch.randn_like(x_start) if self.start_dist == "normal" else 2 * torch.rand_like(x_start) - 1.0
        if self.use_augment and "augment_labels" not in kwargs:
            x_start, kwargs["augment_labels"] = self.augment(x_start, draws=kwargs.pop("augment_draws", None))
        kwargs.pop("augment_draws", None)
        if K is None:
            K = torch.randn_like(x_start)        # (clamped to [-1, 1] where it is read: q_sample and the loss kernel)
        x_start = x_start.to(torch.float32).contiguous()
        noise, K = noise.to(torch.float32).contiguous(), K.to(torch.float32).contiguous()
        t = t.to(torch.float32).contiguous()
        x_noisy = self.q_sample(x_start, noise, t, K)
        theta_pred, noise_pred = self.model(x_noisy, t, **kwargs)
        lpips = self.lpips_active
        if lpips:       # second consumer of both predictions: the gradient sum is ops.fanout's kernel
            theta_pred, theta_lp = ops.fanout(theta_pred, 2)
            noise_pred, noise_lp = ops.fanout(noise_pred, 2)
        B = x_start.shape[0]
        w1, w2 = self.loss_weights(t)
        rec = ((1 - t) ** 2).mean()              # mean_b rec_weight_b^2: the batch-coupled factor of loss_vlb
        w = torch.stack([w1, w2, (rec / B).expand(B)], dim=1).contiguous()
        loss, per_simple, per_mae = ops.ddm_loss_linear(theta_pred, noise_pred, x_start, noise, K, x_noisy, t, w, self.use_l1)
        loss_simple = per_simple.sum() / B
        loss_vlb = per_mae.sum() / B * rec
        if lpips:
            per_lpips = self.perceptual_loss.from_predictions(theta_lp, noise_lp, x_noisy, t, x_start, self._sched)
            lp = per_lpips.sum() / B * rec
            loss = loss + lp
            loss_vlb = loss_vlb + lp.detach()
        log = {"train/loss_simple": loss_simple, "train/loss_vlb": loss_vlb, "train/loss": loss.detach()}
        return loss, log

    def forward(self, x, *args, t: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, **kwargs):
        if args and args[0] is not None:
            raise NotImplementedError("conditional training (`cond`) is not on the unconditional hot path")
        return super().forward(x, t=t, noise=noise, **kwargs)

    # ------------------------------------------------------------------ sampling
    def step_grid(self, denoise=True):
        """The reference's fp32 step sizes (ddm_linear.py:275-280): n steps of 1/n; with `denoise` the last one is split into
        1/n - eps and eps."""
        n = self.sampling_timesteps
        steps = torch.tensor([1.0 / n]).repeat(n)
        if denoise:
            eps = torch.tensor([self._eps_f])
            steps = torch.cat((steps[:-1], steps[-1:] - eps, eps))
        return steps

    def time_grid(self, denoise=True):
        """[(cur_time, s)] per step as the reference's fp32 arithmetic gives them; the last step takes s = cur_time, so the grid
        ends at exactly zero and the last sigma is exactly zero."""
        steps = self.step_grid(denoise)
        cur = torch.ones(())
        out = []
        for i in range(steps.shape[0]):
            s = cur if i == steps.shape[0] - 1 else steps[i]
            out.append((float(cur), float(s)))
            cur = cur - s
        assert float(cur) == 0.0
        return out

    @torch.no_grad()
    def sample(self, batch_size=16, up_scale=1, cond=None, denoise=True, x_T=None, epsilons=None):
        if cond is not None:
            raise NotImplementedError("conditional sampling is not on the unconditional hot path")
        h, w = self.image_size
        return self.sample_fn((batch_size, self.channels, h, w), up_scale=up_scale, unnormalize=True, cond=cond, denoise=denoise,
                              x_T=x_T, epsilons=epsilons)

    @torch.no_grad()
    def sample_fn(self, shape, up_scale=1, unnormalize=True, cond=None, denoise=False, x_T=None, epsilons=None, return_traj=False):
        """Stochastic Euler sampler (ddm_linear.py:272-310): one network evaluation and one fused update launch per step, fp32
        state.  `return_traj`: also the state after every step, the last one before the final clamp."""
        if cond is not None:
            raise NotImplementedError("conditional sampling is not on the unconditional hot path")
        if up_scale != 1:
            raise NotImplementedError("up_scale != 1 (bilinear up-sampling of the start noise) is not implemented")
        dev = self.eps.device
        B = shape[0]
        if x_T is None:
            x_T = self._start_noise(shape, dev)
        img = (x_T.to(device=dev, dtype=torch.float32) * float(self.sigma_max)).contiguous()
        grid = self.time_grid(denoise)
        traj = []
        for k, (cur, s) in enumerate(grid):
            t_vec = torch.full((B,), cur, dtype=torch.float32, device=dev)
            s_vec = torch.full((B,), s, dtype=torch.float32, device=dev)
            theta, noise = self.model(img, t_vec)
            z = (epsilons[k].to(device=dev, dtype=torch.float32) if epsilons is not None
                 else torch.randn(shape, device=dev, dtype=torch.float32)).contiguous()
            last = k == len(grid) - 1
            if return_traj and last:
                traj.append(ops.sampler_step_linear(img.clone(), theta, noise, z, t_vec, s_vec, float(self.scale_input), False))
            ops.sampler_step_linear(img, theta, noise, z, t_vec, s_vec, float(self.scale_input), last and unnormalize)
            if return_traj and not last:
                traj.append(img.clone())
        if not unnormalize:
            img = img.clamp(-self.scale_input, self.scale_input) / self.scale_input
        return (img, traj) if return_traj else img

    def sample_fn_d(self, *a, **k):
        raise NotImplementedError("the linear-drift DDM has the stochastic 'euler' sampler only")

    sample_fn_s = sample_fn_d
