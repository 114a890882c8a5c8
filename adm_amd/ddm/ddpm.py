"""DDM analytic-schedule diffusion wrapper on the HIP hot path.

Mirrors the constructor / ``training_step`` / ``sample`` contract that the reference's drivers call
(SURVEY.md section 8b): ``DDPM(model=unet, cfg=model_cfg, **model_cfg)``,
``training_step(batch) -> (loss, log_dict)``, ``sample(batch_size) -> [B,C,H,W] in [0,1]`` (fp64 for
the deterministic sampler, as the reference returns), buffer ``eps``, attributes ``image_size``,
``channels``.  Skeleton: /root/reference/ddm/ddm_const_2.py:43-389; the 'const' (sqrt t) arithmetic:
/root/reference/ddm/ddm_const.py:284-303, 305-364, 367-476.

Differences, all documented in DESIGN.md:
  * every RNG draw (t, noise, x_T, sampler epsilons) can be injected for parity tests;
  * the LPIPS/VGG16 term (``loss_vlb``, ddm_const.py:351-358 / ddm_const_2.py:242-251) runs on the HIP path
    (adm_amd/ddm/lpips.py) when ``perceptual_weight > 0`` AND its weights were supplied: by the cfg key ``lpips_ckpt``, by
    ``set_perceptual_loss()``, or by a checkpoint whose state dict carries ``perceptual_loss.*``.  No weights ship and none
    are ever fetched; without them the wrapper warns and ``loss_vlb`` is 0;
  * ``use_l1`` in pixel space (per-sample MEAN |.| twins, ddm_const.py:345-348 / ddm_const_2.py:237-240) is one launch of its own
    (``ops.ddm_loss_l1``); a conditional denoiser gets ``batch['cond']`` (ddm_const_2.py:157-161) and ``sample(cond=...)`` runs the
    built-in condition encoder once per call in eval mode, not once per step (same bits);
  * ``use_augment`` runs the AugmentPipe on the GPU (adm_amd/ddm/augment.py) without the reference's per-step host
    read-back of the padding margin; its draws are injectable (``augment_draws=``).
"""
from __future__ import annotations

import warnings
from typing import Optional

import torch
import torch.nn as nn

from .. import ops


def _cfg_get(cfg, key, default):
    if cfg is None:
        return default
    if hasattr(cfg, "get"):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


class DDPMBase(nn.Module):
    SCHEDULE = "const"          # 'const' -> g(t) = sqrt(t) ; 'const_2' -> g(t) = t
    DEFAULT_EPS = 1e-4
    USES_LPIPS = True           # the pixel-space p_losses has the LPIPS term; LatentDiffusion's does not
    AUGMENT_P = 0.15            # AugmentPipe probability multiplier: 0.15 in ddm_const.py:179, 0.12 in ddm_const_2.py:112
    CLIP_IN_SAMPLER = True      # pixel-space 'const' sampler clamps the predicted x0 (ddm_const.py:453-454); latent ones never do
    NO_LPIPS_WARNING = ("adm_amd: the LPIPS term (perceptual_weight > 0) needs VGG16 weights that cannot be fetched "
                        "offline; loss_vlb is 0 (see DESIGN.md)")

    def __init__(self, model, *, image_size, sampling_timesteps=None, loss_type="l2", objective="pred_noise",
                 beta_schedule="cosine", clip_x_start=True, input_keys=("image",), start_dist="normal",
                 sample_type="naive", perceptual_weight=1.0, use_l1=False, **kwargs):
        ckpt_path = kwargs.pop("ckpt_path", None)
        lpips_ckpt = kwargs.pop("lpips_ckpt", None)
        ignore_keys = kwargs.pop("ignore_keys", [])
        only_model = kwargs.pop("only_model", False)
        cfg = kwargs.pop("cfg", None)
        super().__init__()
        self.model = model
        self.channels = self.model.channels
        self.self_condition = self.model.self_condition
        self.input_keys = list(input_keys)
        self.cfg = cfg if cfg is not None else {}
        self.scale_input = _cfg_get(cfg, "scale_input", 1)
        self.register_buffer("eps", torch.tensor(float(_cfg_get(cfg, "eps", self.DEFAULT_EPS))))
        self.sigma_min = _cfg_get(cfg, "sigma_min", 1e-2)
        self.sigma_max = _cfg_get(cfg, "sigma_max", 1)
        self.weighting_loss = _cfg_get(cfg, "weighting_loss", False)
        self.clip_x_start = clip_x_start
        self.image_size = image_size
        self.objective = objective
        if start_dist not in ("normal", "uniform"):
            raise AssertionError("start_dist must be 'normal' or 'uniform'")
        self.start_dist = start_dist
        self.loss_type = loss_type
        self.sampling_timesteps = 10 if sampling_timesteps is None else sampling_timesteps
        self.use_l1 = use_l1        # pixel space: per-sample MEAN |.| twins (ddm_const.py:345-348); latent: sums (ddm_const_2.py:556-559)
        self.perceptual_weight = perceptual_weight
        if lpips_ckpt is None:
            lpips_ckpt = _cfg_get(cfg, "lpips_ckpt", None)
        if perceptual_weight > 0 and self.USES_LPIPS and lpips_ckpt:
            from .lpips import LPIPS
            self.set_perceptual_loss(LPIPS.from_file(lpips_ckpt))
        self.use_augment = bool(_cfg_get(cfg, "use_augment", False))
        if self.use_augment:      # ddm_const.py:179-180 (p = 0.15) / ddm_const_2.py:112-113 (p = 0.12)
            from .augment import AugmentPipe
            self.augment = AugmentPipe(p=self.AUGMENT_P, xflip=1e8, yflip=1, scale=1, rotate_frac=1, aniso=1, translate_frac=1)
        self._eps_f = float(self.eps)
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys, only_model)
        if perceptual_weight > 0 and self.USES_LPIPS and not self.lpips_active:
            warnings.warn(self.NO_LPIPS_WARNING, stacklevel=2)

    # ------------------------------------------------------------------ LPIPS term
    @property
    def lpips_active(self) -> bool:
        """The LPIPS term is computed: perceptual_weight > 0 (a gate, not a factor: ddm_const.py:355) and weights were supplied."""
        return self.USES_LPIPS and self.perceptual_weight > 0 and getattr(self, "perceptual_loss", None) is not None

    def set_perceptual_loss(self, lpips):
        """Install an adm_amd.ddm.lpips.LPIPS instance as the submodule ``perceptual_loss`` (the reference's attribute name).  It is
        frozen: the optimiser, the EMA and the gradient reducer see no new trainable parameter."""
        if not self.USES_LPIPS:
            raise NotImplementedError("the latent p_losses has no LPIPS term")
        for p in lpips.parameters():
            p.requires_grad = False
        self.perceptual_loss = lpips.to(self.eps.device).eval()
        return self

    # ------------------------------------------------------------------ checkpoints
    def init_from_ckpt(self, path, ignore_keys=(), only_model=False, use_ema=False):
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if "ema" in sd and use_ema:
            sd = {(k[10:] if k.startswith("ema_model.") else k): v for k, v in sd["ema"].items()}
        elif "model" in sd:
            sd = sd["model"]
        for k in list(sd.keys()):
            if any(k.startswith(ik) for ik in ignore_keys):
                del sd[k]
        if (self.perceptual_weight > 0 and self.USES_LPIPS and not only_model and getattr(self, "perceptual_loss", None) is None
                and any(k.startswith("perceptual_loss.") for k in sd)):      # a reference-trained checkpoint brings its own VGG16
            from .lpips import LPIPS
            self.set_perceptual_loss(LPIPS.from_state_dict(sd))
        target = self.model if only_model else self
        missing, unexpected = target.load_state_dict(sd, strict=False)
        print(f"Restored from {path} with {len(missing)} missing and {len(unexpected)} unexpected keys")

    # ------------------------------------------------------------------ schedule pieces
    @property
    def _sched(self) -> int:
        return {"const": 0, "const_2": 1, "linear": 2}[self.SCHEDULE]

    def _g(self, t):
        return torch.sqrt(t) if self.SCHEDULE == "const" else t

    def q_sample(self, x_start, noise, t, C=None):
        """x_t = x0 + C t + g(t) eps with C = -x0 (the only C the wrapper ever uses)."""
        return ops.q_sample(x_start, noise, t.to(torch.float32), self._sched)

    def pred_x0_from_xt(self, xt, noise, C, t):
        """x0 = x_t - C t - g(t) eps (ddm_const.py:290-293 / ddm_const_2.py:179-182).  API-parity helper: the samplers
        do this inside their fused HIP step kernels; this standalone form is [B]-broadcast elementwise math."""
        time = t.reshape(C.shape[0], *((1,) * (C.dim() - 1)))
        return xt - C * time - self._g(time) * noise

    def pred_xtms_from_xt(self, xt, noise, C, t, s, epsilon=None):
        """One stochastic reverse step (ddm_const.py:296-303 / ddm_const_2.py:185-197); `epsilon` injectable."""
        time = t.reshape(C.shape[0], *((1,) * (C.dim() - 1)))
        s = s.reshape(C.shape[0], *((1,) * (C.dim() - 1)))
        if self.SCHEDULE == "const":
            mean = xt + C * (time - s) - C * time - s / torch.sqrt(time) * noise
            sigma = torch.sqrt(s * (time - s) / time)
        else:
            mean = xt - C * s - (2 * s * time - s ** 2) / time * noise
            sigma = torch.sqrt(2 * s * time - s ** 2) * (time - s) / time
        if epsilon is None:
            epsilon = torch.randn_like(mean)
        return mean + sigma * epsilon

    def loss_weights(self, t):
        eps = self._eps_f
        if not self.weighting_loss:
            return torch.ones_like(t), torch.ones_like(t)
        if self.SCHEDULE == "const":       # ddm_const.py:336-338
            return (t ** 2 - t + 1) / t, (t ** 2 - t + 1) / (1 - t + eps)
        return ((t - 1) / t) ** 2 + 1, (t / (1 - t + eps)) ** 2 + 1      # ddm_const_2.py:228-230

    # ------------------------------------------------------------------ training
    def get_input(self, batch):
        for k in self.input_keys:
            if k in batch:
                return batch[k]
        return next(iter(batch.values()))

    def training_step(self, batch, *args, **kwargs):
        z = self.get_input(batch)
        cond = batch.get("cond") if hasattr(batch, "get") else None
        if cond is not None:          # conditional denoiser: self(z, cond) -> model(x_t, t, cond)   (ddm_const_2.py:157-161)
            return self(z, cond, *args, **kwargs)
        return self(z, *args, **kwargs)

    def forward(self, x, *args, t: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, **kwargs):
        if self.scale_input != 1:
            x = x * self.scale_input
        if t is None:
            t = torch.rand(x.shape[0], device=x.device) * (1.0 - self._eps_f) + self._eps_f
        return self.p_losses(x, t, *args, noise=noise, **kwargs)

    def p_losses(self, x_start, t, *args, noise: Optional[torch.Tensor] = None, **kwargs):
        if noise is None:
            if self.start_dist == "normal":
                noise = torch.randn_like(x_start)
            else:
                noise = 2 * torch.rand_like(x_start) - 1.0
        if self.use_augment and "augment_labels" not in kwargs:      # ddm_const.py:314-316 / ddm_const_2.py:206-208
            x_start, kwargs["augment_labels"] = self.augment(x_start, draws=kwargs.pop("augment_draws", None))
        kwargs.pop("augment_draws", None)
        x_start = x_start.to(torch.float32).contiguous()
        t = t.to(torch.float32).contiguous()
        x_noisy = self.q_sample(x_start, noise, t)
        C_pred, noise_pred = self.model(x_noisy, t, *args, **kwargs)
        lpips = self.lpips_active
        if lpips:       # the predictions get a second consumer: the gradient sum is ops.fanout's kernel, not autograd's in-place add
            C_pred, C_lp = ops.fanout(C_pred, 2)
            if self.SCHEDULE == "const":
                noise_lp = None          # x_rec = -C_pred (ddm_const.py:326)
            else:
                noise_pred, noise_lp = ops.fanout(noise_pred, 2)
        w1, w2 = self.loss_weights(t)
        w = torch.stack([w1, w2], dim=1).contiguous()
        loss_fn = ops.ddm_loss_l1 if self.use_l1 else ops.ddm_loss
        loss_simple_mean, per_sample = loss_fn(C_pred, noise_pred, x_start, noise, w)
        B, n = x_start.shape[0], x_start[0].numel()
        if lpips:
            # loss_vlb = LPIPS(x_rec, x_start).sum([1,2,3]) * rec_weight is [B] * [B,1] -> [B,B] in the reference, and its sum / B the
            # PRODUCT of the two sums (ddm_const.py:351-358 / ddm_const_2.py:242-251; the same broadcast as the latent L1 term)
            per_lpips = self.perceptual_loss.from_predictions(C_lp, noise_lp, x_noisy, t, x_start, self._sched)
            loss_vlb = per_lpips.sum() * ((-torch.log(t) / 2).sum() / B)
        else:
            loss_vlb = torch.zeros((), device=x_start.device)
        loss = loss_simple_mean + loss_vlb
        log = {"train/loss_simple": per_sample.sum() / B / n,
               "train/loss_vlb": loss_vlb.detach() / n,        # (loss_vlb carries the reference's one / B already)
               "train/loss": loss.detach() / B / n}
        return loss, log

    # ------------------------------------------------------------------ sampling
    def _use_graph(self) -> bool:
        """HIP-graph replay of the sampler's UNet forward (cfg key ``sample_graph`` or ADM_SAMPLE_GRAPH=1).  The forward
        is ~900 launches; at small batch they are launch-bound and a graph removes the per-launch host cost."""
        import os
        return bool(_cfg_get(self.cfg, "sample_graph", False)) or os.environ.get("ADM_SAMPLE_GRAPH", "0") == "1"

    def _sampling_graph(self, shape, dev):
        """Capture (once per shape and weight version) ``C, noise = model(x_static, t_static)``.  Everything inside is
        device-side and allocation-free at the C-ABI level (torch's capture-time allocations come from the graph's private
        pool), so the capture is legal; the fp64 state update stays outside (its t values are host scalars)."""
        from .. import ops
        cache = self.__dict__.setdefault("_graphs", {})
        key = (shape, str(dev))
        ent = cache.get(key)
        if ent is not None and ent["epoch"] == ops._pack_epoch and not self.training:
            return ent
        x = torch.zeros(shape, dtype=torch.float64, device=dev)
        t = torch.ones((), dtype=torch.float64, device=dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):              # warm-up: packs weights, sets kernel attributes, fills allocator pools
            self.model(x, t)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ops.new_amax_pool()                    # the bound vectors of this graph: allocated and zero-filled inside the capture
            C, noise = self.model(x, t)
        ops.new_amax_pool()                        # (eager launches must not write into the graph's private memory)
        ent = {"graph": graph, "x": x, "t": t, "C": C, "noise": noise, "epoch": ops._pack_epoch}
        cache[key] = ent
        return ent

    def _start_noise(self, shape, dev):
        """x_T of the samplers: N(0,1) or U(-1,1) by ``start_dist`` (ddm_const_2.py:305-310, 353-358)."""
        if self.start_dist == "normal":
            return torch.randn(shape, device=dev, dtype=torch.float64)
        return 2 * torch.rand(shape, device=dev, dtype=torch.float64) - 1.0

    def t_steps(self):
        n = self.sampling_timesteps
        i = torch.arange(n, dtype=torch.float64)
        end = self.sigma_min ** 2 if self.SCHEDULE == "const" else 1.0 / n
        ts = self.sigma_max + i / (n - 1) * (end - self.sigma_max)
        return torch.cat([ts, torch.zeros(1, dtype=torch.float64)])

    @torch.no_grad()
    def sample(self, batch_size=16, up_scale=1, cond=None, denoise=True, x_T: Optional[torch.Tensor] = None, epsilons=None):
        if cond is not None:       # ddm_const.py:368-378: the condition sets the batch size
            batch_size = cond[0].shape[0] if isinstance(cond, (list, tuple)) else cond.shape[0]
            cond = self._encode_cond_once(cond)
        h, w = self.image_size
        shape = (batch_size, self.channels, h, w)
        sample_type = _cfg_get(self.cfg, "sample_type", "deterministic")
        if sample_type == "deterministic":
            return self.sample_fn_d(shape, x_T=x_T, cond=cond)
        if sample_type == "stochastic":
            return self.sample_fn_s(shape, x_T=x_T, cond=cond, epsilons=epsilons)
        raise NotImplementedError(sample_type)

    def _encode_cond_once(self, cond):
        """The reference runs the condition encoder on the same photo at every sampler step.  In eval mode it is a pure function of
        the photo, so its four feature maps are computed once per sample() and handed on as the list the denoiser accepts: the same
        bits.  In train mode (stochastic depth draws per call) and without the built-in encoder the per-step call stays."""
        enc = getattr(self.model, "init_conv_mask", None)
        if isinstance(cond, torch.Tensor) and isinstance(enc, nn.Module) and not self.model.training:
            return list(enc(cond))
        return cond

    @torch.no_grad()
    def sample_fn_d(self, shape, up_scale=1, unnormalize=True, cond=None, denoise=False, x_T=None,
                    return_traj=False):
        """10-step deterministic sampler, fp64 state (ddm_const.py:424-476 / ddm_const_2.py:338-389)."""
        dev = self.eps.device
        ts = self.t_steps()
        if x_T is None:
            x_T = self._start_noise(shape, dev)
        x = (x_T.to(device=dev, dtype=torch.float64) * float(ts[0])).contiguous()
        clip = self.clip_x_start and self.SCHEDULE == "const" and self.CLIP_IN_SAMPLER     # const_2 / latent: never clamps x0
        traj = []
        n = len(ts) - 1
        g = self._sampling_graph(tuple(shape), dev) if (self._use_graph() and cond is None) else None
        if g is not None:           # the UNet forward replays from a captured HIP graph on static buffers
            g["x"].copy_(x)
            x = g["x"]
        for i in range(n):
            t_cur, t_next = float(ts[i]), float(ts[i + 1])
            if g is not None:
                g["t"].fill_(t_cur)
                g["graph"].replay()
                C, noise = g["C"], g["noise"]
            elif cond is not None:     # conditional denoiser: model(x, t, cond)  (ddm_const_2.py:712-715)
                C, noise = self.model(x, torch.tensor(t_cur, dtype=torch.float64, device=dev), cond)
            else:
                C, noise = self.model(x, torch.tensor(t_cur, dtype=torch.float64, device=dev))
            last = unnormalize and i == n - 1
            if return_traj and last:   # trajectory holds the pre-normalisation state
                xc = x.clone()
                ops.sampler_step(xc, C, noise, t_cur, t_next, self._sched, clip, float(self.scale_input), False)
                traj.append(xc)
            ops.sampler_step(x, C, noise, t_cur, t_next, self._sched, clip, float(self.scale_input), last)
            if return_traj and not last:
                traj.append(x.clone())
        if g is not None:           # x is the graph's static input buffer: the next sample() of this shape overwrites it
            x = x.clone()
        return (x, traj) if return_traj else x

    @torch.no_grad()
    def sample_fn_s(self, shape, up_scale=1, unnormalize=True, cond=None, denoise=False, x_T=None, epsilons=None):
        """Stochastic sampler (ddm_const.py:380-422 / ddm_const_2.py:288-336) with the per-step update in one HIP
        kernel on an fp64 state.  (The reference promotes to fp64 on its first update anyway -- cur_time is fp64 for
        'const', the state itself for 'const_2' -- so an fp64 state from the start is the same arithmetic.)"""
        dev = self.eps.device
        n = self.sampling_timesteps
        i = torch.arange(n, dtype=torch.float64)
        ts = self.sigma_max ** 2 + i / (n - 1) * (self.sigma_min ** 2 - self.sigma_max ** 2)
        ts = torch.cat([ts, torch.zeros(1, dtype=torch.float64)])
        steps = (-torch.diff(ts)).tolist()
        B = shape[0]
        if x_T is None:
            x_T = self._start_noise(shape, dev)
        img = x_T.to(device=dev, dtype=torch.float64).contiguous()
        if self.SCHEDULE != "const":
            img = img * self.sigma_max
        cur = 1.0
        for k in range(n):
            s = cur if k == n - 1 else steps[k]
            t_vec = torch.full((B,), cur, dtype=torch.float64, device=dev)
            s_vec = torch.full((B,), s, dtype=torch.float64, device=dev)
            C, noise = self.model(img, t_vec, cond) if cond is not None else self.model(img, t_vec)
            z = (epsilons[k].to(device=dev, dtype=torch.float64) if epsilons is not None
                 else torch.randn(shape, device=dev, dtype=torch.float64)).contiguous()
            ops.sampler_step_stochastic(img, C, noise, z, t_vec, s_vec, self._sched, self.clip_x_start,
                                        float(self.scale_input), unnormalize and k == n - 1)
            cur = cur - s
        if not unnormalize:
            img = img.clamp(-self.scale_input, self.scale_input) / self.scale_input
        return img
