"""float64 references of the elementwise / small-reduction operators of adm_amd/csrc/elementwise.hip (schedule, loss, sampler steps,
optimiser, layout movers) and the data the accuracy tests drive them with (a plain helper like fp64ref.py, not a conftest).

Written from the formulas of the reference's modules (ddm_const.py / ddm_const_2.py: q_sample, pred_x0_from_xt, pred_xtms_from_xt,
p_losses; ema.py; torch.optim.AdamW + clip_grad_norm_ as the reference's trainer calls them) on plain torch tensors.  Every function

* takes `dtype`: torch.float64 (the reference) or torch.float32 (plain fp32 torch on the same data: the baseline of bar B);
* returns {output name: (value, mag)}; `mag` is the same formula applied to |operands|, the scale fp64ref.errors() measures against.

Layouts: the schedule / loss / sampler operators take [B, n] (any trailing shape is flattened per sample); activations are NHWC
[B, H, W, C] or NCHW [B, C, H, W] as the kernels have them; per-sample scalars are [B] (or one element, broadcast).
"""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import fill

_f64 = torch.float64


def f32(v):
    """A Python float rounded to float32: what a kernel receives through a C `float` argument."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def _c(t, dtype):
    return None if t is None else t.detach().to(dtype)


def _col(v, like):
    """per-sample scalar [B] (or [1]) as a column against like [B, ...]"""
    return v.reshape(-1, *((1,) * (like.dim() - 1)))


def _gain(schedule, t):
    """noise gain g(t): sqrt(t) for schedule 0 ('const'), t for schedule 1 ('const_2')."""
    return torch.sqrt(t) if schedule == 0 else t


# ------------------------------------------------------------------------------------------------ schedule, loss
def q_sample(x0, noise, t, schedule, dtype=_f64):
    """x_t = x0 + C t + g(t) noise with C = -x0."""
    x0, noise, t = _c(x0, dtype), _c(noise, dtype), _col(_c(t, dtype), x0)
    g = _gain(schedule, t)
    return {"xt": (x0 + (-x0) * t + g * noise, x0.abs() + x0.abs() * t + g * noise.abs())}


def ddm_loss(c_pred, n_pred, x0, noise, w, gscale, dtype=_f64):
    """per[b] = w1 sum (C_pred - C)^2 + w2 sum (noise_pred - noise)^2, C = -x0, w = [B, 2]; d_c, d_n = gscale x its gradients."""
    c, e, x0, noise, w = (_c(v, dtype) for v in (c_pred, n_pred, x0, noise, w))
    w1, w2 = w[:, 0:1], w[:, 1:2]
    e1, e2 = c - (-x0), e - noise
    m1, m2 = c.abs() + x0.abs(), e.abs() + noise.abs()
    return {"per": ((w1 * e1 * e1 + w2 * e2 * e2).sum(1), (w1 * m1 * m1 + w2 * m2 * m2).sum(1)),
            "d_c": (gscale * 2 * w1 * e1, gscale * 2 * w1 * m1),
            "d_n": (gscale * 2 * w2 * e2, gscale * 2 * w2 * m2)}


def ddm_loss_latent(c_pred, n_pred, x0, noise, xt, t, w, gscale, schedule, use_l1, dtype=_f64):
    """LatentDiffusion.p_losses, w = [B, 3] = (w1, w2, w3):

        simple[b] = w1 SSE(C_pred, C) + w2 SSE(noise_pred, noise)                          (use_l1 off)
                  = [w1 (SSE + L1)(C_pred, C) + w2 (SSE + L1)(noise_pred, noise)] / 2      (use_l1 on)
        l1[b]     = sum |x_rec - x0|,   x_rec = x_t - C_pred t - g(t) noise_pred
        d_c, d_n  = gscale x the gradients of  simple[b] + w3 l1[b]          (sign(0) = 0, as torch's abs has it)
    """
    c, e, x0, noise, xt, w = (_c(v, dtype) for v in (c_pred, n_pred, x0, noise, xt, w))
    t = _col(_c(t, dtype), c)
    g = _gain(schedule, t)
    w1, w2, w3 = w[:, 0:1], w[:, 1:2], w[:, 2:3]
    e1, e2 = c - (-x0), e - noise
    m1, m2 = c.abs() + x0.abs(), e.abs() + noise.abs()
    d = xt - c * t - g * e - x0
    dm = xt.abs() + c.abs() * t + g * e.abs() + x0.abs()
    sg = torch.sign(d)
    if use_l1:
        per = ((w1 * (e1 * e1 + e1.abs()) + w2 * (e2 * e2 + e2.abs())) / 2).sum(1)
        perm = ((w1 * (m1 * m1 + m1) + w2 * (m2 * m2 + m2)) / 2).sum(1)
        g1, g2 = (2 * w1 * e1 + w1 * torch.sign(e1)) / 2, (2 * w2 * e2 + w2 * torch.sign(e2)) / 2
        g1m, g2m = (2 * w1 * m1 + w1 * torch.sign(e1).abs()) / 2, (2 * w2 * m2 + w2 * torch.sign(e2).abs()) / 2
    else:
        per, perm = (w1 * e1 * e1 + w2 * e2 * e2).sum(1), (w1 * m1 * m1 + w2 * m2 * m2).sum(1)
        g1, g2, g1m, g2m = 2 * w1 * e1, 2 * w2 * e2, 2 * w1 * m1, 2 * w2 * m2
    return {"per": (per, perm), "l1": (d.abs().sum(1), dm.sum(1)),
            "d_c": (gscale * (g1 - w3 * t * sg), gscale * (g1m + w3 * t * sg.abs())),
            "d_n": (gscale * (g2 - w3 * g * sg), gscale * (g2m + w3 * g * sg.abs()))}


# ------------------------------------------------------------------------------------------------ sampler steps (fp64 state)
# Rounded operations k of each formula, counted beside it; the bar of the fp64 state is 2 k 2^-53 of mag.  The clamps are exact, and
# mag goes through them unclamped (the rounding error of a clamped value is that of its unclamped operands, or 0).
def _finish(x, m, scale_input):
    """the last step's map to [0, 1]: clamp, / scale_input (1 op, skipped for 1.0), (x + 1) / 2 (2 ops)"""
    x = x.clamp(-scale_input, scale_input)
    if scale_input != 1.0:
        x, m = x / scale_input, m / scale_input
    return (x + 1) * 0.5, (m + 1) * 0.5


K_SAMPLER_STEP = 10 + 3          # g(t_cur), g(t_next): 2;  x0: 4;  x_next: 4;  the last step's map: 3


def sampler_step(x, c_pred, n_pred, t_cur, t_next, schedule, clip_x0, scale_input, last, dtype=_f64):
    """x0 = x - C t - g(t) eps [clamped to +-scale_input];  x <- x0 + C t' + g(t') eps  [last: ((clamp(x) / scale_input) + 1) / 2]."""
    x, c, e = _c(x, dtype), _c(c_pred, dtype), _c(n_pred, dtype)
    gc, gn = (math.sqrt(t_cur), math.sqrt(t_next)) if schedule == 0 else (t_cur, t_next)
    x0 = x - c * t_cur - e * gc                                              # 4
    m0 = x.abs() + c.abs() * t_cur + e.abs() * gc
    if clip_x0:
        x0 = x0.clamp(-scale_input, scale_input)
    xn, mn = x0 + c * t_next + e * gn, m0 + c.abs() * t_next + e.abs() * gn     # 4
    if last:
        xn, mn = _finish(xn, mn, scale_input)
    return {"x": (xn, mn)}


K_SAMPLER_STOCHASTIC = {0: 23, 1: 24}
#   const   (0): x0: sqrt, 2 mul, 2 sub = 5;  mean: t - s, 2 mul, add, sub, sqrt, div, mul, sub = 9;  sigma: sub, mul, div, sqrt = 4;
#                sigma z: mul, add = 2;  the last step's map: 3                                                                    -> 23
#   const_2 (1): x0: 4;  mean: C' s, sub, s t (the factor 2 is exact), s s, sub, div, mul, sub = 8;  sigma: s t, s s, sub, sqrt, t - s,
#                mul, div = 7;  sigma z: 2;  the last step's map: 3                                                                -> 24


def sampler_step_stochastic(x, c_pred, n_pred, z, t, s, schedule, clip_x0, scale_input, last, dtype=_f64):
    """pred_xtms_from_xt after pred_x0_from_xt, per sample b with t[b], s[b]:

        x0 = x - C t - g(t) eps  [clamped];  C' = -x0
        const  : mean = x + C' (t - s) - C' t - s / sqrt(t) eps,          sigma = sqrt(s (t - s) / t)
        const_2: mean = x - C' s - (2 s t - s^2) / t eps,                 sigma = sqrt(2 s t - s^2) (t - s) / t
        x <- mean + sigma z   [last: ((clamp(x) / scale_input) + 1) / 2]
    """
    x, c, e, z = (_c(v, dtype) for v in (x, c_pred, n_pred, z))
    t, s = _col(_c(t, dtype), x), _col(_c(s, dtype), x)
    g = _gain(schedule, t)
    x0 = x - c * t - g * e
    m0 = x.abs() + c.abs() * t + g * e.abs()
    if clip_x0:
        x0 = x0.clamp(-scale_input, scale_input)
    c2 = -x0
    if schedule == 0:
        mean = x + c2 * (t - s) - c2 * t - s / torch.sqrt(t) * e
        mm = x.abs() + m0 * (t - s) + m0 * t + s / torch.sqrt(t) * e.abs()
        sigma = torch.sqrt(s * (t - s) / t)
    else:
        mean = x - c2 * s - (2 * s * t - s ** 2) / t * e
        mm = x.abs() + m0 * s + (2 * s * t + s ** 2) / t * e.abs()
        sigma = torch.sqrt(2 * s * t - s ** 2) * (t - s) / t
    xn, mn = mean + sigma * z, mm + sigma * z.abs()
    if last:
        xn, mn = _finish(xn, mn, scale_input)
    return {"x": (xn, mn)}


# ------------------------------------------------------------------------------------------------ optimiser
def sumsq(g, dtype=_f64):
    """sum g^2 (the squared gradient norm before grad_scale)."""
    g = _c(g, dtype)
    s = (g * g).sum()
    return {"sumsq": (s, s)}


def adamw_ema_step(p, g, m, v, ema, *, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=0.0, grad_scale=1.0,
                   ema_decay=None, dtype=_f64):
    """One step of clip_grad_norm_(max_norm) + torch.optim.AdamW + the EMA lerp on tensors:

        norm = |grad_scale g|_2;  clip = min(1, max_norm / (norm + 1e-6)) (1 when max_norm is 0);  g' = clip grad_scale g
        p <- p (1 - lr wd);  m <- b1 m + (1 - b1) g';  v <- b2 v + (1 - b2) g'^2
        p <- p - lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)              (bias corrections in Python floats)
        ema <- ema + (1 - ema_decay) (p - ema)                                              (ema None or ema_decay None: untouched)

    Returns p, m, v, ema (absent without an EMA) and norm."""
    p, g, m, v, ema = (_c(t, dtype) for t in (p, g, m, v, ema))
    b1, b2 = betas
    norm = torch.linalg.vector_norm(g * grad_scale)
    clip = 1.0
    if max_norm > 0:
        clip = min(1.0, max_norm / (float(norm) + 1e-6))
    gs = g * (clip * grad_scale)
    bc1, bc2s = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    p1 = p * (1.0 - lr * weight_decay)
    m2, m2m = b1 * m + (1.0 - b1) * gs, b1 * m.abs() + (1.0 - b1) * gs.abs()
    v2 = b2 * v + (1.0 - b2) * gs * gs
    denom = torch.sqrt(v2) / bc2s + eps
    p2, p2m = p1 - (lr / bc1) * (m2 / denom), p1.abs() + (lr / bc1) * (m2m / denom)
    out = {"p": (p2, p2m), "m": (m2, m2m), "v": (v2, v2), "norm": (norm, norm)}
    if ema is not None:
        if ema_decay is None:
            out["ema"] = (ema, ema.abs())
        else:
            wgt = 1.0 - ema_decay
            out["ema"] = (ema + wgt * (p2 - ema), ema.abs() + wgt * (p2m + ema.abs()))
    return out


# ------------------------------------------------------------------------------------------------ layout + preconditioning
def nchw_to_nhwc(x, mul, cpad, dtype=_f64):
    """y[B, H, W, cpad] = mul[b] x[b, c, h, w] for c < C, 0 in the pad channels; mul [B], [1] or None (1)."""
    x = _c(x, dtype)
    B, C, H, W = x.shape
    k = 1.0 if mul is None else _col(_c(mul, dtype), x)
    y = F.pad((k * x).permute(0, 2, 3, 1), (0, cpad - C))
    return {"y": (y.contiguous(), y.abs().contiguous())}


def precond_out(x, f, a, s, C, dtype=_f64):
    """out[B, C, H, W] = s[b] f[b, h, w, c] + a[b] x[b, c, h, w] (x None: the scaled transpose alone); f has ld >= C channels."""
    f = _c(f, dtype)[..., :C].permute(0, 3, 1, 2)
    y = _col(_c(s, dtype), f) * f
    m = y.abs()
    if x is not None:
        ax = _col(_c(a, dtype), f) * _c(x, dtype)
        y, m = y + ax, m + ax.abs()
    return {"out": (y.contiguous(), m.contiguous())}


def precond_out_bwd(dout, s, ldf, dtype=_f64):
    """df[B, H, W, ldf] = s[b] dout[b, c, h, w] for c < C, 0 in the pad channels (s None: 1)."""
    return {"df": nchw_to_nhwc(dout, s, ldf, dtype)["y"]}


def axpby_b(x, y, a, s, dtype=_f64):
    """out = s[b] y + a[b] x (x None: s[b] y)."""
    y = _c(y, dtype)
    o = _col(_c(s, dtype), y) * y
    m = o.abs()
    if x is not None:
        ax = _col(_c(a, dtype), y) * _c(x, dtype).reshape(y.shape)
        o, m = o + ax, m + ax.abs()
    return {"out": (o, m)}


def resample2x(x, mode, scale, prefill=None, dtype=_f64):
    """NHWC: mode 0: scale x the sum of each 2x2 block; mode 1: scale x nearest-neighbour x2; prefill (acc = 1) is added."""
    x = _c(x, dtype)
    if mode == 0:
        y = (x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2]) * scale
        m = (x.abs()[:, 0::2, 0::2] + x.abs()[:, 0::2, 1::2] + x.abs()[:, 1::2, 0::2] + x.abs()[:, 1::2, 1::2]) * abs(scale)
    else:
        y = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) * scale
        m = y.abs()
    if prefill is not None:
        y, m = y + _c(prefill, dtype), m + _c(prefill, dtype).abs()
    return {"y": (y, m)}


def concat2(a, b, scale_b, dtype=_f64):
    """y = (a | scale_b b) along the last axis."""
    y = torch.cat([_c(a, dtype), _c(b, dtype) * scale_b], dim=-1)
    return {"y": (y, y.abs())}


def split2(dy, ca, scale_b, dtype=_f64):
    """da = dy[..., :ca], db = scale_b dy[..., ca:]."""
    dy = _c(dy, dtype)
    da, db = dy[..., :ca].contiguous(), (dy[..., ca:] * scale_b).contiguous()
    return {"da": (da, da.abs()), "db": (db, db.abs())}


def copy_channels(src, src_off, dst, dst_off, C, scale, acc, dtype=_f64):
    """dst[:, dst_off : dst_off + C] = scale src[:, src_off : src_off + C] (+ what dst held, acc = 1); the rest of dst stays."""
    src, dst = _c(src, dtype), _c(dst, dtype).clone()
    mag = dst.abs()
    v = src[:, src_off:src_off + C] * scale
    old = dst[:, dst_off:dst_off + C]
    dst[:, dst_off:dst_off + C] = v + old if acc else v
    mag[:, dst_off:dst_off + C] = v.abs() + old.abs() if acc else v.abs()
    return {"dst": (dst, mag)}


def add(a, b, c=None, dtype=_f64):
    """a + b (+ c)."""
    ts = [_c(t, dtype) for t in (a, b, c) if t is not None]
    return {"y": (sum(ts[1:], ts[0]), sum((t.abs() for t in ts[1:]), ts[0].abs()))}


def silu(x, dy=None, dtype=_f64):
    """y = x sigmoid(x); given dy, dx = dy s (1 + x (1 - s)), s = sigmoid(x).  mag: |y|, |dy| s (1 + |x| (1 - s))."""
    x = _c(x, dtype)
    s = torch.sigmoid(x)
    out = {"y": (x * s, (x * s).abs())}
    if dy is not None:
        d = _c(dy, dtype)
        out["dx"] = (d * s * (1 + x * (1 - s)), d.abs() * s * (1 + x.abs() * (1 - s)))
    return out


def pos_embedding(t, C, dtype=_f64):
    """PositionalEmbedding (max_positions 10000, endpoint off): f_k = 10000^(-k / (C / 2)), emb = (cos(t f) | sin(t f)), [B, C]."""
    t = _c(t, dtype).reshape(-1)
    half = C // 2
    fr = (1.0 / 10000.0) ** (torch.arange(half, dtype=dtype, device=t.device) / half)
    ang = torch.outer(t, fr)
    y = torch.cat([torch.cos(ang), torch.sin(ang)], dim=1)
    return {"emb": (y, torch.ones_like(y))}       # (no sums: the scale of a cosine's rounding error is 1)


# ------------------------------------------------------------------------------------------------ sizes and data
CAP_THREADS = 8192 * 256          # ew_grid: at most 8192 workgroups of 256


def wrap_size(k, mult4=False):
    """Elements of a launch whose threads make a second (partial, ragged) trip of the grid-stride loop: k = elements per thread."""
    return CAP_THREADS * k + 256 * k * 3 + (4 if mult4 else 3)


WRAP_1 = wrap_size(1)             # kernels of one element per thread
WRAP_B3 = (WRAP_1 + 2) // 3 + 1   # ... as the per-sample n of a B = 3 launch: 3 n >= WRAP_1 and no multiple of 4; the end of sample 2 lies beyond the first trip
WRAP_ADAMW = wrap_size(4)
WRAP_SUMSQ = wrap_size(16)
WRAP_X4 = wrap_size(1)            # f32x4 kernels: this many 16-byte vectors
RAGGED_N = 1009                   # per sample; B = 3: 3027 elements, no multiple of 4 / 64 / 256, sample boundaries inside a wave

_BLOCK = (1 << 20) + 7            # the period of tiled data (odd: no period of the launch geometry divides it)


def data(shape, tag, scale=1.0, dtype=torch.float32):
    """oracle.fill.hash_tensor, tiled from a block of 2^20 + 7 values above that size (the hash costs 80 ns an element)."""
    n = math.prod(shape)
    if n <= 2 * _BLOCK:
        return fill.hash_tensor(tuple(shape), tag, scale, dtype)
    blk = fill.hash_tensor((_BLOCK,), tag, scale, dtype)
    return blk.repeat((n + _BLOCK - 1) // _BLOCK)[:n].reshape(shape).contiguous()


T_CASES = (1e-4, 0.23, 0.999, 1.0)            # q_sample


def t_triples():
    """B = 3 time vectors that together hold T_CASES, each with three distinct values."""
    return [torch.tensor(v, dtype=torch.float32) for v in ((1e-4, 0.23, 0.999), (1.0, 1e-4, 0.23), (0.999, 1.0, 0.5))]


LOSS_T = (1e-4, 0.999, 0.37)                  # per sample: the weights span loss_weights(t = 1e-4) ... loss_weights(t = 0.999)
# Samples of a loss case.  The per-sample sums are B numbers, each with the rounding of its final f32 value (uniform in +- half an ulp),
# and the samples near t = 1e-4 (w1 = 1e4) carry all of rms(mag): bar B's e_rms <= 2 e_rms(fp32 torch) compares two such roundings, and
# with one dominant sample a correctly rounded sum misses it one time in four.  24 samples = 8 near each t make e_rms a statistic.
LOSS_B = 24
LOSS_EPS = 1e-4
LOSS_NS = (RAGGED_N, 65536, 65537, 3 * 256 * 256)


def loss_weights(schedule, t):
    """(w1, w2, w3) [B, 3] float32 from the reference's weighting (eps 1e-4) and rec_weight = -log(t) / 2."""
    t = t.double()
    if schedule == 0:
        w1, w2 = (t ** 2 - t + 1) / t, (t ** 2 - t + 1) / (1 - t + LOSS_EPS)
    else:
        w1, w2 = ((t - 1) / t) ** 2 + 1, (t / (1 - t + LOSS_EPS)) ** 2 + 1
    return torch.stack([w1, w2, -torch.log(t) / 2], dim=1).float()


@functools.lru_cache(maxsize=None)
def loss_data(n, schedule):
    """(shared between tests: read only)  c_pred, n_pred, x0, noise, xt [B, n], t [B], w [B, 3] with B = LOSS_B; t[b] = LOSS_T[b % 3]
    (1 - 0.003 (b // 3)): distinct per sample.  Every 11th element has C_pred = -x0 and every 13th noise_pred = noise
    (the L1 twins' arguments are exactly 0); every 17th has C_pred = noise_pred = 0 and x_t = x0 (x_rec - x0 is exactly 0 in any
    arithmetic).  Elsewhere x_t = x0 + C_pred t + g noise_pred + delta with 0.01 <= |delta| <= 1.01, so the sign of x_rec - x0 is not
    a matter of rounding."""
    B = LOSS_B
    c, e, x0, noise = (data((B, n), f"loss.{nm}", sc) for nm, sc in (("c", 1.0), ("e", 1.3), ("x0", 1.0), ("noise", 1.7)))
    t = torch.tensor([LOSS_T[b % 3] * (1 - 0.003 * (b // 3)) for b in range(B)], dtype=torch.float32)
    i = torch.arange(n)
    c[:, i % 11 == 3] = -x0[:, i % 11 == 3]
    e[:, i % 13 == 5] = noise[:, i % 13 == 5]
    z = i % 17 == 7
    c[:, z] = 0.0
    e[:, z] = 0.0
    dl = data((B, n), "loss.delta", 1.0)
    dl = dl + 0.01 * torch.where(dl >= 0, 1.0, -1.0)
    td = t.double().reshape(B, 1)
    xt = (x0.double() + c.double() * td + _gain(schedule, td) * e.double() + dl.double()).float()
    xt[:, z] = x0[:, z]
    return dict(c=c, e=e, x0=x0, noise=noise, xt=xt, t=t, w=loss_weights(schedule, t))


SAMPLER_STEPS = ((0.6, 0.45), (0.3, 0.0), (1e-4, 0.0))                  # (t_cur, t_next): a middle step, t_next = 0, the step from 1e-4
SCALE_INPUTS = (1.0, 0.987654321)
# per-sample (t, s) of the stochastic step, s <= t: a middle step, s == t exactly (the sampler's last step), t = 1e-4
STOCH_TS = (((1.0, 0.11), (0.37, 0.37), (1e-4, 1e-4)),
            ((1e-4, 2.5e-5), (0.89, 0.11), (0.5, 0.5)))


def sampler_data(n, B=3):
    """x, z fp64 and C_pred, noise_pred fp32, [B, n]."""
    return dict(x=data((B, n), "smp.x", 1.7, _f64), z=data((B, n), "smp.z", 2.5, _f64),
                c=data((B, n), "smp.c", 1.0), e=data((B, n), "smp.e", 1.7))


ADAM_STEPS = (1, 2, 10, 1000, 100000)
ADAM_LR = 1e-2


def adam_data(n):
    """p (|p| around 0.05), g, m, v > 0 and an ema that differs from p: float32 [n]."""
    g = data((n,), "adam.g", 0.02)
    return dict(p=data((n,), "adam.p", 0.1), g=g, m=data((n,), "adam.m", 0.01),
                v=(data((n,), "adam.v", 2e-4).abs() + 1e-6), ema=data((n,), "adam.ema", 0.1))


ADAM_N = 3 * RAGGED_N
# (step, max_norm, grad_scale, weight_decay, ema): ema "none" = no EMA buffer, None = buffer left alone, else the decay.  With adam_data
# the norm of grad_scale g is 0.64 (grad_scale 1) or 0.08 (1 / 8) at ADAM_N: max_norm 10 is above both (clip = 1), 0.05 below both.
ADAM_CASES = ((1, 0.0, 1.0, 0.0, "none"), (1, 10.0, 1.0, 1e-2, 0.9996), (2, 0.05, 1.0, 1e-2, 0.0), (2, 0.0, 0.125, 0.0, 0.9996),
              (10, 0.05, 0.125, 1e-2, None), (10, 10.0, 0.125, 0.0, 0.0), (1000, 0.05, 1.0, 0.0, 0.9996), (1000, 0.0, 1.0, 1e-2, "none"),
              (100000, 10.0, 1.0, 1e-2, 0.9996), (100000, 0.05, 0.125, 0.0, None))
ADAM_WRAP_CASE = (1000, 1.0, 1.0, 1e-2, 0.9996)          # at WRAP_ADAMW elements (norm 33: clipped)


def adam_ref(d, case, dtype=_f64):
    """adamw_ema_step on adam_data for one of the cases above (the float arguments as the kernel receives them: rounded to float32)."""
    step, max_norm, gscale, wd, ema = case
    return adamw_ema_step(d["p"], d["g"], d["m"], d["v"], None if ema == "none" else d["ema"], step=step, lr=ADAM_LR, eps=1e-8,
                          weight_decay=wd, max_norm=max_norm, grad_scale=gscale, ema_decay=None if ema == "none" else ema, dtype=dtype)
