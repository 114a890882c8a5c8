"""fp64 references of the conv, attention and GroupNorm operators and of the SR denoiser's own family (weight standardisation, channel
LayerNorm, BatchNorm, bilinear resize, the generic multi-head and the linear attention, SpatialAtt, activations, Fourier features,
col2im), for the accuracy tests (a plain helper like parity.py, not a conftest).

Layouts are the kernels': activations NHWC [B, H, W, C], weights OIHW [Co, Ci, k, k] (or [Co, Ci] for a Linear), attention qkv
[B, L, heads * 192] with each head's 192 channels packed as (q[64] | k[64] | v[64]) and its output [B, L, heads * 64].

Every contraction is written as shifted matmuls in float64 (torch.matmul on whatever device the inputs are on: no dependence on a
double-precision convolution library); the gradients are those matmuls' own backward.  Each result comes with `mag`, the same
operation applied to |operands| -- sum |a b| per output element -- which is the scale a rounding error is measured against:

    e_max = max |got - ref| / max mag,        e_rms = rms(got - ref) / rms(mag)          (errors())
"""
import math

import torch
import torch.nn.functional as F

_f64 = torch.float64


def _taps(x, w, stride, pad):
    """sum over the k x k taps of (shifted, strided view of the padded x) @ w[:, :, i, j]^T."""
    k = w.shape[-1]
    lo, hi = pad
    B, H, W, _ = x.shape
    xp = F.pad(x, (0, 0, lo, hi, lo, hi))
    Ho, Wo = (H + lo + hi - k) // stride + 1, (W + lo + hi - k) // stride + 1
    y = None
    for i in range(k):
        for j in range(k):
            xs = xp[:, i:i + stride * (Ho - 1) + 1:stride, j:j + stride * (Wo - 1) + 1:stride, :]
            t = torch.matmul(xs, w[:, :, i, j].t())
            y = t if y is None else y + t
    return y


def conv_fwd(x, w, *, up=False, stride=1, pad=None):
    """NHWC conv, fp64: optional fused nearest x2 up-sampling of x, a stride, and (lo, hi) zero padding (default k // 2 each side)."""
    if w.dim() == 2:
        w = w[:, :, None, None]
    if up:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    k = w.shape[-1]
    return _taps(x, w, stride, (k // 2, k // 2) if pad is None else tuple(pad))


def conv(x, w, b=None, res=None, dy=None, *, up=False, stride=1, pad=None):
    """{"y": (ref, mag)} and, given dy, also "dx", "dw" and (with a bias) "db" of y = conv(x, w) + b + res.  Inputs of any float dtype
    (x NHWC with exactly Ci channels, dy with exactly Co); everything is computed in float64 on x's device."""
    x, w = x.to(_f64), w.to(_f64)
    out = {}
    for part in ("ref", "mag"):
        a = (lambda t: t.abs()) if part == "mag" else (lambda t: t)
        xa, wa = a(x).detach().requires_grad_(dy is not None), a(w).detach().requires_grad_(dy is not None)
        y = conv_fwd(xa, wa, up=up, stride=stride, pad=pad)
        if b is not None:
            y = y + a(b.to(_f64))
        if res is not None:
            y = y + a(res.to(_f64))
        res_ = {"y": y.detach()}
        if dy is not None:
            g = a(dy.to(_f64))
            dx, dw = torch.autograd.grad(y, (xa, wa), g)
            res_.update(dx=dx, dw=dw)
            if b is not None:
                res_["db"] = g.sum(dim=(0, 1, 2))
        for n, t in res_.items():
            out.setdefault(n, [None, None])[0 if part == "ref" else 1] = t
    return {n: tuple(v) for n, v in out.items()}


def attention(qkv, heads, dout=None):
    """{"out": (ref, mag)} and, given dout, "dqkv" of softmax(q k^T / 8) v per head, in the layout of ops.attention.  mag applies
    the same products to |operands| with the (non-negative) softmax weights P kept: out -> P |v|; dv -> P^T |dout|;
    dP -> |dout| |v|^T; dS -> P (|dP| + rowsum(P |dP|)); dq -> |dS| |k| / 8; dk -> |dS|^T |q| / 8."""
    shp = qkv.shape
    B, L = shp[0], math.prod(shp[1:-1])
    t = qkv.to(_f64).reshape(B, L, heads, 3, 64).permute(3, 0, 2, 1, 4)          # [3][B][heads][L][64]
    q, k, v = t[0], t[1], t[2]
    P = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) / 8.0, dim=-1)
    o = torch.matmul(P, v)
    to_out = lambda u: u.permute(0, 2, 1, 3).reshape(*shp[:-1], heads * 64)
    res = {"out": (to_out(o), to_out(torch.matmul(P, v.abs())))}
    if dout is None:
        return res
    do = dout.to(_f64).reshape(B, L, heads, 64).permute(0, 2, 1, 3)
    dP = torch.matmul(do, v.transpose(-1, -2))
    dS = P * (dP - (dP * P).sum(-1, keepdim=True))
    dPm = torch.matmul(do.abs(), v.abs().transpose(-1, -2))
    dSm = P * (dPm + (dPm * P).sum(-1, keepdim=True))
    grads = []
    for S, qq, kk, dd in ((dS, q, k, do), (dSm, q.abs(), k.abs(), do.abs())):
        dq = torch.matmul(S, kk) / 8.0
        dk = torch.matmul(S.transpose(-1, -2), qq) / 8.0
        dv = torch.matmul(P.transpose(-1, -2), dd)
        grads.append(torch.stack([dq, dk, dv], dim=3).permute(0, 2, 1, 3, 4).reshape(shp))     # [B][L][heads][3][64]
    res["dqkv"] = tuple(grads)
    return res


def group_norm(x, gamma, beta, ss, *, groups, eps, silu, keep=None, addend=None, dy=None):
    """{"y": (ref, mag)} and, given dy, "dx", "dgamma", "dbeta" and (with ss) "dss" of ops.group_norm_act / group_norm_act_fork:

        xhat = (x - mean_g) rstd_g,  z = xhat gamma + beta,  u = (1 + s) z + t,  y = act(u) keep

    x NHWC [B, H, W, C]; group g = channels [g cpg, (g + 1) cpg) of one image, biased variance; ss = [B, 2C] or [1, 2C] rows of
    (s | t) or None; keep = the dropout mask already divided by 1 - p; addend = the fork's residual gradient, added to dx.  Written
    from the definition in float64 on x's device; the gradients are autograd's on that graph.  mag: |y|; for the parameter gradients
    the same sums over |summands|; for dx (= rstd (gamma' du - mean_g(gamma' du) - xhat mean_g(gamma' du xhat)) + addend, gamma' =
    gamma (1 + s), du = dy keep act'(u)):  rstd (|gamma' du| + mean_g |gamma' du| + |xhat| mean_g |gamma' du xhat|) + |addend|."""
    need = dy is not None
    x = x.detach().to(_f64).requires_grad_(need)
    gamma, beta = (t.detach().to(device=x.device, dtype=_f64).requires_grad_(need) for t in (gamma, beta))
    B, H, W, C = x.shape
    cpg = C // groups
    xg = x.reshape(B, H * W, groups, cpg)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = (xg - mean).square().mean(dim=(1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = ((xg - mean) * rstd).reshape(B, H, W, C)
    z = xhat * gamma + beta
    u, sc1 = z, None
    if ss is not None:
        ss = ss.detach().to(device=x.device, dtype=_f64).requires_grad_(need)
        sc1 = 1.0 + ss[:, :C].reshape(-1, 1, 1, C)
        u = sc1 * z + ss[:, C:].reshape(-1, 1, 1, C)
    y = u * torch.sigmoid(u) if silu else u
    if keep is not None:
        y = y * keep.to(device=x.device, dtype=_f64)
    out = {"y": (y.detach(), y.detach().abs())}
    if not need:
        return out
    dy = dy.to(device=x.device, dtype=_f64)
    wrt = [x, gamma, beta, u] + ([ss] if ss is not None else [])
    g = torch.autograd.grad(y, wrt, dy)
    dx, du = g[0], g[3]                                        # du = dy keep act'(u)
    zd, xh = z.detach(), xhat.detach()
    dz = du if sc1 is None else du * sc1.detach()              # (1 + s) du
    gdu = (dz * gamma.detach()).abs()                          # |gamma' du|
    gmean = lambda t: t.reshape(B, H * W, groups, cpg).mean(dim=(1, 3), keepdim=True).expand(B, H * W, groups, cpg).reshape(B, H, W, C)
    rs = rstd.detach().expand(B, H * W, groups, cpg).reshape(B, H, W, C)
    dx_mag = rs * (gdu + gmean(gdu) + xh.abs() * gmean(gdu * xh.abs()))
    if addend is not None:
        a = addend.to(device=x.device, dtype=_f64)
        dx, dx_mag = dx + a, dx_mag + a.abs()
    out["dx"] = (dx, dx_mag)
    out["dgamma"] = (g[1], (dz * xh).abs().sum(dim=(0, 1, 2)))
    out["dbeta"] = (g[2], dz.abs().sum(dim=(0, 1, 2)))
    if ss is not None:
        m = torch.cat([(du * zd).abs().sum(dim=(1, 2)), du.abs().sum(dim=(1, 2))], dim=1)        # [B, 2C]
        out["dss"] = (g[4], m if ss.shape[0] == B else m.sum(dim=0, keepdim=True))
    return out


# ------------------------------------------------------------------------------------------------ the SR denoiser's family
def _d(t, like=None):
    return t.detach().to(device=t.device if like is None else like.device, dtype=_f64)


def weight_std(w, eps=1e-5, dy=None):
    """{"y": (ref, mag)} and, given dy, "dw" of ops_cond.weight_standardize: per row o of w [O, ...] (K values),
    y = (w - mean_o) rstd_o, rstd = (biased var + eps)^-1/2.  mag: |y|;  dw = rstd (dy - mean(dy) - y mean(dy y)) -> rstd (|dy| +
    mean |dy| + |y| mean |dy y|)."""
    w = _d(w)
    r = w.reshape(w.shape[0], -1)
    mean = r.mean(dim=1, keepdim=True)
    var = (r - mean).square().mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (r - mean) * rstd
    out = {"y": (y.reshape(w.shape), y.abs().reshape(w.shape))}
    if dy is not None:
        g = _d(dy, w).reshape(r.shape)
        m = lambda t: t.mean(dim=1, keepdim=True)
        dw = rstd * (g - m(g) - y * m(g * y))
        dm = rstd * (g.abs() + m(g.abs()) + y.abs() * m((g * y).abs()))
        out["dw"] = (dw.reshape(w.shape), dm.reshape(w.shape))
    return out


def layer_norm_c(x, g, eps=1e-5, dy=None):
    """{"y"} and, given dy, "dx", "dg" of ops_cond.layer_norm_c: per pixel of x [..., C], y = (x - mean_c) rstd g (gain only, biased
    variance).  mag: |y|; dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)) -> the same sum over |terms|; dg = sum_pixels dy xhat
    -> sum |dy xhat|."""
    x = _d(x)
    C = x.shape[-1]
    g = _d(g, x).reshape(C)
    mean = x.mean(dim=-1, keepdim=True)
    var = (x - mean).square().mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    y = xh * g
    out = {"y": (y, y.abs())}
    if dy is not None:
        d = _d(dy, x)
        gd = d * g
        m = lambda t: t.mean(dim=-1, keepdim=True)
        out["dx"] = (rstd * (gd - m(gd) - xh * m(gd * xh)), rstd * (gd.abs() + m(gd.abs()) + xh.abs() * m((gd * xh).abs())))
        out["dg"] = ((d * xh).reshape(-1, C).sum(dim=0), (d * xh).abs().reshape(-1, C).sum(dim=0))
    return out


def batch_norm(x, gamma, beta, run_mean, run_var, *, training, momentum, eps, dy=None):
    """{"y", "running_mean", "running_var"} and, given dy, "dx", "dgamma", "dbeta" of ops_cond.batch_norm on x [..., C] (M rows).
    training: batch mean and biased variance normalise, the running statistics move by `momentum` towards the batch mean and the
    UNBIASED variance; eval: the running statistics normalise and stay, and they are constants of the backward (dx = gamma rstd dy).
    mag: y -> |xhat gamma| + |beta|; running_mean -> (1 - m) |run_mean| + m mean |x|; running_var -> itself (a sum of squares);
    dx = gamma rstd (dy - mean(dy) - xhat mean(dy xhat)) -> the sum over |terms|; dgamma = sum dy xhat, dbeta = sum dy -> sums of
    |summands|."""
    x = _d(x)
    C = x.shape[-1]
    r = x.reshape(-1, C)
    M = r.shape[0]
    gamma, beta, rm, rv = (_d(t, x).reshape(C) for t in (gamma, beta, run_mean, run_var))
    if training:
        mean = r.mean(dim=0)
        var = (r - mean).square().mean(dim=0)
        new_rm = (1 - momentum) * rm + momentum * mean
        new_rv = (1 - momentum) * rv + momentum * var * (M / max(M - 1, 1))
        rm_mag = (1 - momentum) * rm.abs() + momentum * r.abs().mean(dim=0)
    else:
        mean, var, new_rm, new_rv, rm_mag = rm, rv, rm, rv, rm.abs()
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (r - mean) * rstd
    y = xh * gamma + beta
    out = {"y": (y.reshape(x.shape), ((xh * gamma).abs() + beta.abs()).reshape(x.shape)),
           "running_mean": (new_rm, rm_mag), "running_var": (new_rv, new_rv.abs())}
    if dy is not None:
        d = _d(dy, x).reshape(-1, C)
        m = lambda t: t.mean(dim=0, keepdim=True)
        if training:
            dx = gamma * rstd * (d - m(d) - xh * m(d * xh))
            dm = gamma.abs() * rstd * (d.abs() + m(d.abs()) + xh.abs() * m((d * xh).abs()))
        else:
            dx = gamma * rstd * d
            dm = dx.abs()
        out["dx"] = (dx.reshape(x.shape), dm.reshape(x.shape))
        out["dgamma"] = ((d * xh).sum(dim=0), (d * xh).abs().sum(dim=0))
        out["dbeta"] = (d.sum(dim=0), d.abs().sum(dim=0))
    return out


def bilinear_matrix(n_in, n_out, align_corners, device=None):
    """[n_out, n_in] fp64 interpolation matrix of one axis from explicit source coordinates: align_corners: s = d (in - 1) / (out - 1)
    (0 for out = 1); else s = max(0, (d + 1/2) in / out - 1/2); i0 = floor(s), i1 = min(i0 + 1, in - 1), weights 1 - (s - i0), s - i0."""
    d = torch.arange(n_out, dtype=_f64, device=device)
    if align_corners:
        s = d * ((n_in - 1) / (n_out - 1)) if n_out > 1 else torch.zeros_like(d)
    else:
        s = ((d + 0.5) * (n_in / n_out) - 0.5).clamp_min(0.0)
    i0 = s.floor().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    lam = s - i0
    R = torch.zeros(n_out, n_in, dtype=_f64, device=device)
    rows = torch.arange(n_out, device=device)
    R.index_put_((rows, i0.long()), 1.0 - lam, accumulate=True)
    R.index_put_((rows, i1.long()), lam, accumulate=True)
    return R


def bilinear(x, Ho, Wo, align_corners, dy=None):
    """{"y"} and, given dy, "dx" of ops_cond.bilinear on NHWC x: y = Ry x Rx^T with the two axis matrices of bilinear_matrix, dx =
    Ry^T dy Rx.  The weights are non-negative: mag is the same map applied to |x| (|dy|)."""
    x = _d(x)
    Ry = bilinear_matrix(x.shape[1], Ho, align_corners, x.device)
    Rx = bilinear_matrix(x.shape[2], Wo, align_corners, x.device)
    f = lambda t: torch.einsum("oh,bhwc,pw->bopc", Ry, t, Rx)
    out = {"y": (f(x), f(x.abs()))}
    if dy is not None:
        d = _d(dy, x)
        b = lambda t: torch.einsum("oh,bopc,pw->bhwc", Ry, t, Rx)
        out["dx"] = (b(d), b(d.abs()))
    return out


def mha(q, k, v, heads, scale, dout=None):
    """{"out": (ref, mag)} and, given dout, "dq", "dk", "dv" of ops_cond.mha: softmax(scale q k^T) v per head; q [B, Lq, heads D],
    k, v [B, Lk, heads D], head h in columns [h D, (h + 1) D).  mag as in attention(): the softmax weights P kept, every product on
    |operands|."""
    B, Lq, C = q.shape
    Lk, D = k.shape[1], C // heads
    hd = lambda t, L: _d(t, q).reshape(B, L, heads, D).permute(0, 2, 1, 3)
    un = lambda t, L: t.permute(0, 2, 1, 3).reshape(B, L, C)
    qq, kk, vv = hd(q, Lq), hd(k, Lk), hd(v, Lk)
    P = torch.softmax(torch.matmul(qq, kk.transpose(-1, -2)) * scale, dim=-1)
    res = {"out": (un(torch.matmul(P, vv), Lq), un(torch.matmul(P, vv.abs()), Lq))}
    if dout is None:
        return res
    do = hd(dout, Lq)
    dP = torch.matmul(do, vv.transpose(-1, -2))
    dS = P * (dP - (dP * P).sum(-1, keepdim=True))
    dPm = torch.matmul(do.abs(), vv.abs().transpose(-1, -2))
    dSm = P * (dPm + (dPm * P).sum(-1, keepdim=True))
    res["dq"] = (un(torch.matmul(dS, kk) * scale, Lq), un(torch.matmul(dSm, kk.abs()) * abs(scale), Lq))
    res["dk"] = (un(torch.matmul(dS.transpose(-1, -2), qq) * scale, Lk), un(torch.matmul(dSm.transpose(-1, -2), qq.abs()) * abs(scale), Lk))
    res["dv"] = (un(torch.matmul(P.transpose(-1, -2), do), Lk), un(torch.matmul(P.transpose(-1, -2), do.abs()), Lk))
    return res


def mha_packed(qkv, heads, scale, dout=None):
    """mha() on the packed layout of ops_cond.self_attention_packed: qkv [B, L, 3 C] = (q | k | v), row stride 3 C; {"out"} and,
    given dout, "dqkv" in the same layout."""
    C = qkv.shape[-1] // 3
    r = mha(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads, scale, dout)
    res = {"out": r["out"]}
    if dout is not None:
        res["dqkv"] = tuple(torch.cat([r[n][i] for n in ("dq", "dk", "dv")], dim=-1) for i in (0, 1))
    return res


def linear_attention(qkv, dout=None, heads=4):
    """{"out"} and, given dout, "dqkv" of ops_cond.linear_attention on qkv [B, N, 3 heads D] = (q | k | v):

        qs = softmax_d(q) D^-1/2,  ks = softmax_n(k),  ctx[d][e] = sum_n ks[n][d] v[n][e] / N,  out[n][e] = sum_d ctx[d][e] qs[n][d]

    The softmax weights qs, ks (non-negative) stay as they are in mag; every other product is taken on |operands|:
    dctx = qs^T dout; dqs = dout ctx^T; dq = qs (dqs - sum_d dqs softmax_d(q)) -> qs (|dqs| + sum ...);  dv = ks dctx / N;
    dks = v dctx^T / N;  dk = ks (dks - sum_n ks dks) -> ks (|dks| + sum_n ks |dks|)."""
    B, N, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    t = _d(qkv).reshape(B, N, 3, heads, D).permute(2, 0, 3, 1, 4)                # [3][B][heads][N][D]
    q, k, v = t[0], t[1], t[2]
    qsm = torch.softmax(q, dim=-1)
    qs = qsm * D ** -0.5
    ks = torch.softmax(k, dim=-2)
    un = lambda u: u.permute(0, 2, 1, 3).reshape(B, N, C)
    T = lambda u: u.transpose(-1, -2)
    ctx, ctxm = torch.matmul(T(ks), v) / N, torch.matmul(T(ks), v.abs()) / N      # [B][heads][D][D]
    res = {"out": (un(torch.matmul(qs, ctx)), un(torch.matmul(qs, ctxm)))}
    if dout is None:
        return res
    do = _d(dout, qkv).reshape(B, N, heads, D).permute(0, 2, 1, 3)
    grads = []
    for mag in (False, True):
        a = (lambda u: u.abs()) if mag else (lambda u: u)
        sg = 1.0 if mag else -1.0
        dctx = torch.matmul(T(qs), a(do))
        dqs = torch.matmul(a(do), T(ctxm if mag else ctx))
        dq = qs * (a(dqs) + sg * (a(dqs) * qsm).sum(-1, keepdim=True))
        dv = torch.matmul(ks, dctx) / N
        dks = torch.matmul(a(v), T(dctx)) / N
        dk = ks * (a(dks) + sg * (ks * a(dks)).sum(-2, keepdim=True))
        grads.append(torch.cat([un(dq), un(dk), un(dv)], dim=-1))
    res["dqkv"] = tuple(grads)
    return res


def spatial_att_gate(att, qk, h, xres, dy=None):
    """{"y"} and, given dy, "dh", "datt", "dqk" of ops_cond.spatial_att_gate.  a = channel 0 of att [B, H, W, ld]; qk = (qw, qb, kw,
    kb); q_i = qw a_i + qb, k_j = kw a_j + kb, P = softmax_j(q_i k_j), av = P a, g = av / (1 + |av|), y = g h + xres.
    datt is [B, H, W, ld] with channels 1.. zero.  mag keeps P: y -> |g h| + |xres|; dg_i = sum_c dy h -> sum |dy h|;
    dav = dg / (1 + |av|)^2; dS_ij = P_ij dav_i (a_j - av_i) -> P |dav| (|a_j| + P |a|); dq = dS k, dk = dS^T q,
    datt = P^T dav + qw dq + kw dk, dqk = (dq . a, sum dq, dk . a, sum dk): each on |terms|."""
    h = _d(h)
    B, H, W, C = h.shape
    HW = H * W
    a = _d(att, h).reshape(B, HW, -1)[:, :, 0]
    qw, qb, kw, kb = (float(t) for t in qk.detach().double().reshape(-1))
    q, k = qw * a + qb, kw * a + kb
    P = torch.softmax(q[:, :, None] * k[:, None, :], dim=-1)
    av = torch.matmul(P, a[:, :, None])[:, :, 0]
    g = av / (1 + av.abs())
    hh, xr = h.reshape(B, HW, C), _d(xres, h).reshape(B, HW, C)
    y = g[:, :, None] * hh + xr
    out = {"y": (y.reshape(h.shape), ((g[:, :, None] * hh).abs() + xr.abs()).reshape(h.shape))}
    if dy is None:
        return out
    d = _d(dy, h).reshape(B, HW, C)
    out["dh"] = ((g[:, :, None] * d).reshape(h.shape), (g[:, :, None] * d).abs().reshape(h.shape))
    datt, dqk = [], []
    for mag in (False, True):
        f = (lambda u: u.abs()) if mag else (lambda u: u)
        dg = f(d * hh).sum(-1)
        dav = dg / (1 + av.abs()).square()
        if mag:
            avm = torch.matmul(P, a.abs()[:, :, None])[:, :, 0]
            dS = P * dav[:, :, None] * (a.abs()[:, None, :] + avm[:, :, None])
        else:
            dS = P * dav[:, :, None] * (a[:, None, :] - av[:, :, None])
        dq = torch.matmul(dS, f(k)[:, :, None])[:, :, 0]
        dk = torch.matmul(dS.transpose(-1, -2), f(q)[:, :, None])[:, :, 0]
        da = torch.matmul(P.transpose(-1, -2), dav[:, :, None])[:, :, 0] + (abs(qw) if mag else qw) * dq + (abs(kw) if mag else kw) * dk
        full = torch.zeros(B, HW, att.shape[-1], dtype=_f64, device=h.device)
        full[:, :, 0] = da
        datt.append(full.reshape(att.shape))
        dqk.append(torch.stack([(dq * f(a)).sum(), dq.sum(), (dk * f(a)).sum(), dk.sum()]))
    out["datt"], out["dqk"] = tuple(datt), tuple(dqk)
    return out


def recover_keep(y, y0):
    """The dropout mask a kernel applied, from its output y and the undropped fp64 output y0: an element was dropped where y is 0 and
    y0 is not (an element whose undropped value is 0 counts as kept: it is 0 either way)."""
    return ((y.detach().to(y0.device) != 0) | (y0 == 0)).to(_f64)


def act(x, kind, keep=None, dy=None):
    """{"y"} and, given dy, "dx" of ops_cond.relu_dropout / gelu / dropout: y = f(x) keep, dx = dy f'(x) keep; kind "relu", "gelu"
    (the exact erf form) or "id"; keep = the dropout mask already divided by 1 - p (recover_keep(...) / (1 - p)).  mag: |y|, |dx|."""
    x = _d(x)
    if kind == "relu":
        y, dv = x.clamp_min(0.0), (x > 0).to(_f64)
    elif kind == "gelu":
        cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
        y, dv = x * cdf, cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    else:
        assert kind == "id"
        y, dv = x, torch.ones_like(x)
    kp = 1.0 if keep is None else _d(keep, x)
    y = y * kp
    out = {"y": (y, y.abs())}
    if dy is not None:
        dx = _d(dy, x) * dv * kp
        out["dx"] = (dx, dx.abs())
    return out


def fourier_features(x, W):
    """{"y"} of ops_cond.fourier_features: [sin(2 pi x_b W_d) | cos(2 pi x_b W_d)], [B, 2 D].  No sums: mag is |y| (its maximum, which
    errors() divides by, is 1 for all practical inputs)."""
    p = _d(x).reshape(-1, 1) * _d(W, x).reshape(1, -1) * (2.0 * math.pi)
    y = torch.cat([torch.sin(p), torch.cos(p)], dim=-1)
    return {"y": (y, y.abs())}


def col2im(col, B, Hin, Win, ks, stride, pad):
    """{"dx"} of adm_col2im: the adjoint of the strided gather col[b][oy][ox][ky ks + kx][c] = xpad[b][stride oy + ky - pad][stride ox
    + kx - pad][c] (zero outside the map), i.e. every col entry added to the pixel it was gathered from.  col [B, Ho, Wo, ks ks, C].
    mag: the same sums over |col|."""
    col = _d(col)
    Ho, Wo, C = col.shape[1], col.shape[2], col.shape[-1]
    Hp, Wp = max(Hin + 2 * pad, stride * (Ho - 1) + ks), max(Win + 2 * pad, stride * (Wo - 1) + ks)
    res = []
    for c in (col, col.abs()):
        c = c.reshape(B, Ho, Wo, ks, ks, C)
        xp = torch.zeros(B, Hp, Wp, C, dtype=_f64, device=col.device)
        for ky in range(ks):
            for kx in range(ks):
                xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :] += c[:, :, :, ky, kx, :]
        res.append(xp[:, pad:pad + Hin, pad:pad + Win, :].contiguous())
    return {"dx": tuple(res)}


# ------------------------------------------------------------------------------------------------ the Swin condition encoder's family
def _ln_rows(x, w, b, eps, dy):
    """LayerNorm with weight and bias over the last axis of fp64 x: (y, y_mag, xh, rstd) and, given dy, (dx, dx_mag, dw, dw_mag, db,
    db_mag).  y = xh w + b -> |xh w| + |b|; dx = rstd (g - mean g - xh mean(g xh)), g = dy w -> the same sum over |terms|; dw = sum_rows
    dy xh, db = sum_rows dy -> sums of |summands|."""
    C = x.shape[-1]
    mean = x.mean(dim=-1, keepdim=True)
    var = (x - mean).square().mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    fwd = (xh * w + b, (xh * w).abs() + b.abs(), xh, rstd)
    if dy is None:
        return fwd, None
    g = dy * w
    m = lambda t: t.mean(dim=-1, keepdim=True)
    dx = rstd * (g - m(g) - xh * m(g * xh))
    dxm = rstd * (g.abs() + m(g.abs()) + xh.abs() * m((g * xh).abs()))
    r = lambda t: t.reshape(-1, C).sum(dim=0)
    return fwd, (dx, dxm, r(dy * xh), r((dy * xh).abs()), r(dy), r(dy.abs()))


def layer_norm_affine(x, w, b, eps=1e-5, dy=None):
    """{"y"} and, given dy, "dx", "dw", "db" of ops_swin.layer_norm (adm_ln_affine_fwd / _bwd): nn.LayerNorm(C) with weight and bias over
    the rows of x [..., C], biased variance.  mag as in _ln_rows.  The results keep x's row layout, so a test can take errors() over a
    class of rows."""
    x = _d(x)
    fwd, bwd = _ln_rows(x, _d(w, x), _d(b, x), eps, None if dy is None else _d(dy, x))
    out = {"y": fwd[:2]}
    if bwd is not None:
        out.update(dx=bwd[0:2], dw=bwd[2:4], db=bwd[4:6])
    return out


def merge_index(H, W, Cin, device=None):
    """The PatchMerging gather as index arithmetic: for output row (oy, ox) and channel c of 4 Cin, quad = c // Cin, ci = c % Cin, the
    source pixel is (2 oy + (quad & 1), 2 ox + (quad >> 1)) -- quads in the order (0,0), (1,0), (0,1), (1,1) as (dy, dx).  Returns
    (iy [Ho, 1, 4Cin], ix [1, Wo, 4Cin], ci [4Cin], inside [Ho, Wo, 4Cin])."""
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    c = torch.arange(4 * Cin, device=device)
    quad, ci = c // Cin, c % Cin
    iy = 2 * torch.arange(Ho, device=device).reshape(Ho, 1, 1) + (quad & 1).reshape(1, 1, -1)
    ix = 2 * torch.arange(Wo, device=device).reshape(1, Wo, 1) + (quad >> 1).reshape(1, 1, -1)
    return iy, ix, ci, (iy < H) & (ix < W)


def merge_layer_norm(x, w, b, eps=1e-5, dy=None):
    """{"y"} and, given dy, "dx", "dw", "db" of ops_swin.merge_layer_norm: x [B, H, W, Cin] -> the 2x2 gather of merge_index (zeros
    past an odd edge, which count in the mean's divisor 4 Cin) -> LayerNorm(4 Cin).  dx goes back through the same gather: every source
    pixel has one destination, a position past the edge none.  mag as in _ln_rows."""
    x = _d(x)
    B, H, W, Cin = x.shape
    iy, ix, ci, inside = merge_index(H, W, Cin, x.device)
    Ho, Wo = iy.shape[0], ix.shape[1]
    xp = torch.zeros(B, 2 * Ho, 2 * Wo, Cin, dtype=_f64, device=x.device)
    xp[:, :H, :W] = x
    g = xp[:, iy, ix, ci]                                          # [B, Ho, Wo, 4 Cin]
    fwd, bwd = _ln_rows(g, _d(w, x), _d(b, x), eps, None if dy is None else _d(dy, x))
    out = {"y": fwd[:2]}
    if bwd is not None:
        back = []
        for t in bwd[0:2]:
            full = torch.zeros_like(xp)
            full[:, iy, ix, ci] = t
            back.append(full[:, :H, :W].contiguous())
        out.update(dx=tuple(back), dw=bwd[2:4], db=bwd[4:6])
    return out


SWIN_WIN, SWIN_HEAD_DIM = 7, 32


def window_index(H, W, shift, device=None):
    """The shifted-window partition as index arithmetic.  shift = (sh, sw); an axis whose padded size is one window takes no shift.
    Rolled-frame coordinate r = w 7 + t, source coordinate (padded frame) s = (r + shift) mod P, region label along an axis with a shift
    (r >= P - 7) + (r >= P - shift).  Returns (Y, X [windows, 49] source coordinates of token t = ty 7 + tx of every window (row-major
    windows), lab [windows, 49] = 3 ly + lx, rel [49, 49] = (dy + 6) 13 + (dx + 6) with (dy, dx) = query - key position, (sh, sw) used)."""
    Wn = SWIN_WIN
    Ph, Pw = -(-H // Wn) * Wn, -(-W // Wn) * Wn
    sh, sw = (shift, shift) if isinstance(shift, int) else shift
    sh, sw = (sh if Ph > Wn else 0), (sw if Pw > Wn else 0)

    def axis(P, s):
        r = torch.arange(P, device=device)
        lab = torch.zeros(P, dtype=torch.long, device=device) if s == 0 else (r >= P - Wn).long() + (r >= P - s).long()
        return (r + s) % P, lab

    (sy, ly), (sx, lx) = axis(Ph, sh), axis(Pw, sw)
    nh, nw = Ph // Wn, Pw // Wn
    rows = lambda t: t.reshape(nh, 1, Wn, 1).expand(nh, nw, Wn, Wn).reshape(nh * nw, Wn * Wn)
    cols = lambda t: t.reshape(1, nw, 1, Wn).expand(nh, nw, Wn, Wn).reshape(nh * nw, Wn * Wn)
    p = torch.arange(Wn * Wn, device=device)
    py, px = p // Wn, p % Wn
    rel = (py[:, None] - py[None, :] + Wn - 1) * (2 * Wn - 1) + (px[:, None] - px[None, :] + Wn - 1)
    return rows(sy), cols(sx), rows(ly) * 3 + cols(lx), rel, (sh, sw)


def window_attention(qkv, qkv_bias, table, heads, shift, dout=None):
    """{"out"} and, given dout, "d_qkv", "d_table", "d_qkv_bias" of ops_swin.window_attention (adm_swin_attn_fwd / _bwd): qkv [B, H, W,
    3C] with the last axis ordered [3][heads][32], qkv_bias [3C], table [169, heads], shift an int or (sh, sw).  Per window and head

        S = 32^-1/2 q k^T + table[rel][head] - 100 [labels differ],  P = softmax(S),  O = P v

    over the 49 tokens of window_index; a token outside H x W is a key / value equal to qkv_bias and is never a query (its dout is 0).
    dP = dO v^T, dS = P (dP - rowsum(P dP)), dq = 32^-1/2 dS k, dk = 32^-1/2 dS^T q, dv = P^T dO; d_qkv takes them at the real tokens,
    d_qkv_bias the sums of dk, dv (and dq, which is zero) over the padding tokens, d_table[rel] the sums of dS.
    mag keeps P (non-negative) and takes every other product on |operands|: out -> P |v|; dP -> |dO| |v|^T; dS -> P (|dP| + rowsum(P
    |dP|)); dq, dk, dv, d_table and d_qkv_bias -> the same sums over |summands|."""
    qkv = _d(qkv)
    dev = qkv.device
    B, H, W, C3 = qkv.shape
    C, D, T = C3 // 3, SWIN_HEAD_DIM, SWIN_WIN * SWIN_WIN
    assert C == heads * D
    Y, X, lab, rel, _ = window_index(H, W, shift, dev)
    nW = Y.shape[0]
    Ph, Pw = int(Y.max()) + 1, int(X.max()) + 1
    real = ((Y < H) & (X < W)).to(_f64)                                     # [nW, 49]
    bias = _d(qkv_bias, qkv)
    full = bias.expand(B, Ph, Pw, C3).clone()
    full[:, :H, :W] = qkv
    tok = full[:, Y, X].reshape(B, nW, T, 3, heads, D).permute(3, 0, 1, 4, 2, 5)      # [3][B][nW][heads][49][32]
    q, k, v = tok[0], tok[1], tok[2]
    scale = D ** -0.5
    tb = _d(table, qkv)[rel].permute(2, 0, 1)                               # [heads, 49, 49]
    mask = (lab[:, :, None] != lab[:, None, :]).to(_f64) * -100.0          # [nW, 49, 49]
    S = scale * torch.matmul(q, k.transpose(-1, -2)) + tb + mask[:, None]
    P = torch.softmax(S, dim=-1)

    def to_map(t, ch):          # [B][nW][heads][49][32] per third -> [B, H, W, ch]
        m = torch.zeros(B, Ph, Pw, ch, dtype=_f64, device=dev)
        m[:, Y, X] = t
        return m[:, :H, :W].contiguous()

    tokens = lambda t: t.permute(0, 1, 3, 2, 4).reshape(B, nW, T, C)       # heads next to the channel
    res = {"out": (to_map(tokens(torch.matmul(P, v)), C), to_map(tokens(torch.matmul(P, v.abs())), C))}
    if dout is None:
        return res
    dfull = torch.zeros(B, Ph, Pw, C, dtype=_f64, device=dev)
    dfull[:, :H, :W] = _d(dout, qkv)
    do = dfull[:, Y, X].reshape(B, nW, T, heads, D).permute(0, 1, 3, 2, 4)
    Tr = lambda t: t.transpose(-1, -2)
    dP = torch.matmul(do, Tr(v))
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    dPm = torch.matmul(do.abs(), Tr(v.abs()))
    dSm = P * (dPm + (P * dPm).sum(-1, keepdim=True))
    outs = {"d_qkv": [], "d_table": [], "d_qkv_bias": []}
    for s_, qq, kk, dd in ((dS, q, k, do), (dSm, q.abs(), k.abs(), do.abs())):
        thirds = torch.cat([tokens(scale * torch.matmul(s_, kk)), tokens(scale * torch.matmul(Tr(s_), qq)),
                            tokens(torch.matmul(Tr(P), dd))], dim=-1)      # [B, nW, 49, 3C]
        outs["d_qkv"].append(to_map(thirds, C3))
        outs["d_qkv_bias"].append((thirds * (1.0 - real)[None, :, :, None]).sum(dim=(0, 1, 2)))
        dt = torch.zeros(rel.max().item() + 1, heads, dtype=_f64, device=dev)
        dt.index_add_(0, rel.reshape(-1), s_.sum(dim=(0, 1)).reshape(heads, T * T).t().contiguous())
        outs["d_table"].append(dt)
    res.update({n: tuple(v_) for n, v_ in outs.items()})
    return res


def patch_embed_ln(x, w, cb, gamma, beta, eps=1e-5, dy=None):
    """{"y"} and, given dy, "dW", "db", "dgamma", "dbeta" of ops_swin's fused one-channel stem (adm_patch_embed_ln_fwd / _bwd):
    x [B, 1, H, W] -> the 4x4 patches p [B, H//4, W//4, 16] (trailing rows / columns unread) -> c = p w^T + cb with w [E, 1, 4, 4]
    -> LayerNorm over E with gamma, beta.  There is no dx.  mag: c -> |p| |w|^T + |cb|; y = (c - mean c) rstd gamma + beta ->
    rstd |gamma| (mag c + mean mag c) + |beta|; dgamma = sum dy xh, dbeta = sum dy -> sums of |summands|; dc = rstd (g - mean g - xh
    mean(g xh)), g = dy gamma -> the sum over |terms|; db = sum_tokens dc, dW = dc^T p -> the same sums over |dc| terms and |p|."""
    x = _d(x)
    B, _, H, W = x.shape
    Ht, Wt = H // 4, W // 4
    E = w.shape[0]
    p = x[:, 0, :4 * Ht, :4 * Wt].reshape(B, Ht, 4, Wt, 4).permute(0, 1, 3, 2, 4).reshape(B, Ht, Wt, 16)
    wm, cbv, ga, be = _d(w, x).reshape(E, 16), _d(cb, x), _d(gamma, x), _d(beta, x)
    c = torch.matmul(p, wm.t()) + cbv
    cm = torch.matmul(p.abs(), wm.abs().t()) + cbv.abs()
    m = lambda t: t.mean(dim=-1, keepdim=True)
    mean = m(c)
    rstd = 1.0 / torch.sqrt(m((c - mean).square()) + eps)
    xh = (c - mean) * rstd
    out = {"y": (xh * ga + be, rstd * ga.abs() * (cm + m(cm)) + be.abs())}
    if dy is None:
        return out
    d = _d(dy, x)
    g = d * ga
    dc = rstd * (g - m(g) - xh * m(g * xh))
    dcm = rstd * (g.abs() + m(g.abs()) + xh.abs() * m((g * xh).abs()))
    r = lambda t: t.reshape(-1, E).sum(dim=0)
    P2 = p.reshape(-1, 16)
    out["dgamma"] = (r(d * xh), r((d * xh).abs()))
    out["dbeta"] = (r(d), r(d.abs()))
    out["db"] = (r(dc), r(dcm))
    out["dW"] = (torch.matmul(dc.reshape(-1, E).t(), P2).reshape(w.shape), torch.matmul(dcm.reshape(-1, E).t(), P2.abs()).reshape(w.shape))
    return out


def row_scale_add(x, r, s):
    """{"y"} of ops_swin.row_scale_add (adm_rowscale_add): y[b] = x[b] + s[b] r[b], or s[b] r[b] when x is None.  A sample with
    s[b] == 0 copies x (so a -0.0 stays -0.0) or, without x, is +0.0.  From fp32 operands the fp64 value is the exact product plus one
    rounding: rounded once more to fp32 it is what one fused multiply-add gives."""
    r_ = _d(r)
    sv = _d(s, r).reshape(-1, *([1] * (r_.dim() - 1)))
    if x is None:
        y = torch.where(sv == 0, torch.zeros_like(r_), sv * r_)
        return {"y": (y, y.abs())}
    x_ = _d(x, r)
    y = torch.where(sv == 0, x_, x_ + sv * r_)
    return {"y": (y, x_.abs() + (sv * r_).abs())}


def errors(got, ref, mag):
    """(e_max, e_rms) of got against the fp64 reference, relative to max / rms of mag (0 where mag is all zero and got exact)."""
    d = got.detach().to(device=ref.device, dtype=_f64) - ref
    m_max, m_rms = float(mag.abs().max()), float(mag.double().square().mean().sqrt())
    e_max, e_rms = float(d.abs().max()), float(d.square().mean().sqrt())
    return (e_max / m_max if m_max > 0 else (0.0 if e_max == 0 else math.inf),
            e_rms / m_rms if m_rms > 0 else (0.0 if e_rms == 0 else math.inf))


def bar_b(e, e32):
    """Bar B (a split format against the f32-MFMA kernel on the same data): e_rms <= 2 e_rms(f32) + 1e-9 and
    e_max <= max(2 e_max(f32), 4e-7).  Returns (passes, ratio_max, ratio_rms): ratios of the errors to their limits."""
    r_max = e[0] / max(2.0 * e32[0], 4e-7)
    r_rms = e[1] / (2.0 * e32[1] + 1e-9)
    return r_max <= 1.0 and r_rms <= 1.0, r_max, r_rms
