"""fp64 references of the conv, attention and GroupNorm operators, for the accuracy tests (a plain helper like parity.py, not a conftest).

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
