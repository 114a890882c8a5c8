"""The case table of the SR denoiser's kernel family (csrc/cond_ops.hip, csrc/attention_small.hip), its data, the fp64 reference and
the fp32 torch composition of every case, shared by tests/test_fp64ref_cond_host.py (CPU) and tests/test_hip_cond_accuracy.py (GPU).
A plain helper like gn_cases.py, not a conftest.

CASES[op] is a list of tuples whose first entry is the case's name; the comment behind a row says which code path it is there for.
make(op, case) gives the case's CPU fp32 tensors (fixed generator, cached, shared: do not modify), reference(op, case, data, ...) the
fp64ref dict on the data's device, torch32(op, case, data, ...) the same outputs from plain fp32 torch on the CPU (the comparator of
the fallback bar) -- with `defect=` one deliberate mistake, for the teeth tests.

FALLBACK names the cases in which plain fp32 arithmetic itself cannot be expected to meet BAR_A (fp32 torch is above BAR_A / 4 on at
least one output: tests/test_fp64ref_cond_host.py asserts that the set is exactly those cases).  There the limit of the GPU test is
max(BAR_A, 2 x e_max of fp32 torch on the same data).

Data kinds of the normalisers (x = std * randn + mean):
    plain    std 2, mean 0.3 (WS: weight scale 0.3, mean 0.05)
    eps      variance ~ eps of the operator, so that eps carries half of rstd (WS: weight scale 3e-3, LN: std 3e-3, BN: std 0.03)
    const    the eps data with row / channel 0 exactly constant (0.75: any fp32 sum of it is exact)
    offset   |mean| / std = 15 (the GroupNorm tests' offset data)
"""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

import fp64ref

WS_EPS, LN_EPS, BN_EPS, BN_MOMENTUM = 1e-5, 1e-5, 1e-3, 0.03
DROP_SEED = 20240611

CASES = {
    # (name, O, ci, k, kind): rows of K = ci k k values, one workgroup of 256 threads per row
    "ws": [
        ("K63-eps", 5, 7, 3, "eps"),                     # K < 256: idle threads
        ("K63-offset", 5, 7, 3, "offset"),
        ("K96-plain", 6, 96, 1, "plain"),                # a 1x1 weight
        ("K288-const", 8, 32, 3, "const"),               # K > 256: the second trip of the row loop is partial
        ("K1152-eps", 4, 128, 3, "eps"),                 # the recipe's 128 -> 128 3x3
        ("K2304-offset", 3, 256, 3, "offset"),
    ],
    # (name, M, C, kind): M pixel rows; forward one wave per row; backward ceil(M / 256) workgroups (cap 2048) + colpart_final
    "ln": [
        ("M1-C4-const", 1, 4, "const"),                  # one row, one quad
        ("M3-C12-eps", 3, 12, "eps"),
        ("M257-C384-eps", 257, 384, "eps"),              # 2 workgroups in the backward
        ("M257-C1024-const", 257, 1024, "const"),        # the widest row: 4 quads per lane
        ("M300-C128-plain", 300, 128, "plain"),
        ("M513-C128-offset", 513, 128, "offset"),        # 3 workgroups
        ("M524800-C4-eps", 524800, 4, "eps"),            # > 2048 x 256 rows: past the workgroup cap, 8 MB
    ],
    # (name, M, C, kind, training): ceil(M / 512) workgroups (cap 1024) of partial moments + finalize, forward and backward
    "bn": [
        ("M1-C12-eval-plain", 1, 12, "plain", False),
        ("M3-C1024-train-plain", 3, 1024, "plain", True),
        ("M257-C384-train-offset", 257, 384, "offset", True),
        ("M513-C4-train-eps", 513, 4, "eps", True),              # 2 workgroups of 257 and 256 rows (rows are split evenly)
        ("M1025-C12-train-const", 1025, 12, "const", True),      # 3 workgroups of 342, 342 and 341 rows
        ("M1025-C128-eval-eps", 1025, 128, "eps", False),        # running variance ~ eps
        ("M513-C384-eval-offset", 513, 384, "offset", False),
        ("M524800-C4-train-offset", 524800, 4, "offset", True),  # past the 1024-workgroup cap: 1023 workgroups of 513 rows, the last of 1
        ("M8200-C512-train-plain", 8200, 512, "plain", True),    # 1 049 600 quads: the grid-stride loop of bn_apply and bn_bwd_dx
    ],
    # (name, B, Hi, Wi, Ho, Wo, C, align_corners, into): into = None or (coff, ld) for bilinear_into
    "bilinear": [
        ("up-4x4-9x7-T", 2, 4, 4, 9, 7, 8, True, None),
        ("up-8x8-32x32-F", 2, 8, 8, 32, 32, 8, False, None),
        ("down-16x12-5x7-T", 2, 16, 12, 5, 7, 8, True, None),
        ("down-32x32-8x8-F", 1, 32, 32, 8, 8, 8, False, None),
        ("down-9x14-4x5-F", 2, 9, 14, 4, 5, 4, False, None),
        ("1x1-8x8-T", 2, 1, 1, 8, 8, 8, True, None),
        ("1x1-5x3-F", 2, 1, 1, 5, 3, 8, False, None),
        ("same-6x10-T", 2, 6, 10, 6, 10, 8, True, None),
        ("same-6x10-F", 2, 6, 10, 6, 10, 8, False, None),
        ("up-3x5-9x4-F", 2, 3, 5, 9, 4, 12, False, None),
        ("Hi128-300x3-T", 1, 128, 2, 300, 3, 4, True, None),     # the f32 source coordinate is least exact at Hi = 128
        ("Hi128-300x3-F", 1, 128, 2, 300, 3, 4, False, None),
        ("C384-2x2-5x5-T", 1, 2, 2, 5, 5, 384, True, None),      # the backward's one-row thread map (R = 2)
        ("into-coff3-T", 2, 4, 4, 8, 8, 8, True, (3, 16)),       # the stem: behind 3 latent channels, scalar stores
        ("into-coff8-F", 2, 4, 4, 8, 8, 8, False, (8, 24)),      # a float4-aligned slice
        ("grid-8x8-260x260-T", 1, 8, 8, 260, 260, 64, True, None),   # 1 081 600 quads: the forward's grid-stride loop
    ],
    # (name, shape, kind, drop_p): kind relu / gelu / id
    "act": [
        ("relu", (2, 5, 7, 12), "relu", 0.0),
        ("relu-drop", (2, 16, 16, 32), "relu", 0.1),
        ("gelu", (2, 9, 9, 16), "gelu", 0.0),
        ("dropout", (2, 16, 16, 32), "id", 0.2),
        ("grid-relu-drop", (1, 1024, 1025, 4), "relu", 0.1),     # 1 049 600 quads: the grid-stride loop
    ],
    # (name, B, D, kind): kind "wide" = the recipe's log-times x N(0, 16^2) frequencies, "small" = phases below 1, "mid" = phases of
    # a few turns (up to ~ 10 radians: the argument reduction of sinf / cosf works, the fp32 phase is still good to 1e-6)
    "fourier": [
        ("small-D16", 5, 16, "small"),
        ("mid-D64", 6, 64, "mid"),
        ("wide-D16", 7, 16, "wide"),
        ("wide-D300", 3, 300, "wide"),                   # more than one workgroup
    ],
    # (name, B, Hin, Win, C, ks, stride, pad): Ho = (Hin + 2 pad - ks) // stride + 1
    "col2im": [
        ("down-8x12", 2, 8, 12, 8, 4, 2, 1),             # Downsample = Conv2d(C, C', 4, 2, 1)
        ("down-9x7", 2, 9, 7, 8, 4, 2, 1),               # odd map: the last row / column is gathered by fewer taps
        ("stem-6x5", 1, 6, 5, 4, 7, 1, 3),               # the 7x7 stem
        ("k3s1-5x5", 1, 5, 5, 4, 3, 1, 1),
        ("grid-130x130", 1, 130, 130, 256, 2, 2, 0),     # 1 081 600 quads: the grid-stride loop
    ],
    # (name, B, Lq, Lk, heads, D, scale, kind, packed): one thread per query (key), 64-row tiles.  kind: plain; x6 = every input
    # times 6 (logits of a few hundred at scale 1, RelationNet has no 1 / sqrt(d)); equal = all keys identical; dominant = one key
    # far above the rest in every row
    "mha": [
        ("Lq1-Lk1-D16", 2, 1, 1, 8, 16, 1.0, "plain", False),
        ("Lq16-Lk1024-D16", 1, 16, 1024, 8, 16, 1.0, "plain", False),        # the recipe's cross-attention, 16 key tiles
        ("Lq63-Lk64-D16-x6", 1, 63, 64, 8, 16, 1.0, "x6", False),
        ("Lq64-Lk65-D32", 1, 64, 65, 8, 32, 1.0, "plain", False),            # a second key tile of one row
        ("Lq65-Lk63-D64-x6", 1, 65, 63, 8, 64, 1.0, "x6", False),            # a second query tile of one row
        ("Lq130-Lk130-D32-x6", 1, 130, 130, 8, 32, 1.0, "x6", False),        # Lq > 64 with a partial last tile
        ("Lq16-Lk130-D64-soft", 1, 16, 130, 8, 64, 1.0, "soft", False),      # q, k times 1/2: a flat softmax at D = 64
        ("Lq65-Lk130-D16-equal", 1, 65, 130, 8, 16, 1.0, "equal", False),    # uniform softmax
        ("Lq70-Lk130-D32-dominant", 1, 70, 130, 8, 32, 1.0, "dominant", False),
        ("packed-L256-D32", 1, 256, 256, 4, 32, 32 ** -0.5, "plain", True),  # the bottleneck Attention, ld = 3 C
        ("packed-L65-D32-x6", 2, 65, 65, 4, 32, 32 ** -0.5, "x6", True),
    ],
    # (name, B, N, kind): ceil(N / 1024) chunks of 64-row tiles; kind spread = k columns over +-30 with the maximum late in the map
    "la": [
        ("N1", 2, 1, "plain"),
        ("N63", 2, 63, "plain"),
        ("N65-spread", 2, 65, "spread"),                 # a second tile of one row
        ("N1025-spread", 1, 1025, "spread"),             # two chunks (513 + 512 rows): the first one's last tile has one row
        ("N1025", 2, 1025, "plain"),
        ("N16384", 1, 16384, "plain"),                   # the recipe's 128 x 128 map: 16 chunks
    ],
    # (name, B, H, W, C, (qw, qb, kw, kb), att_scale): the recomputing kernel of ops_cond._SpatialAttBig, one workgroup per image
    "spatt": [
        ("hw1", 2, 1, 1, 8, (0.7, 0.1, -0.5, 0.2), 1.0),
        ("hw257-qw-pos", 2, 257, 1, 8, (0.7, 0.1, 0.9, -0.2), 1.0),          # a second trip of every 256-thread loop
        ("hw257-qw-neg", 1, 257, 1, 64, (-0.8, 0.3, 0.6, 0.1), 1.0),         # rows whose maximum sits at the smallest k
        ("hw257-qw-zero", 1, 257, 1, 8, (0.0, 0.4, 0.6, 0.1), 1.0),
        ("hw2560", 1, 64, 40, 8, (0.5, 0.1, -0.4, 0.2), 1.0),                # the largest map the kernel takes
        ("hw300-saturated", 1, 20, 15, 8, (0.3, 0.1, 0.2, 0.0), 30.0),       # |av| ~ 30: the softsign is flat
    ],
}

# cases on the fallback bar: max(BAR_A, 2 x fp32 torch).  Why plain fp32 cannot meet BAR_A there:
#   bn offset, M = 524 800       x - mean cancels 4 bits and half a million such terms per channel follow
#   mha x6                       a logit of a few hundred carries an absolute error of ~ 1e-5, which exp() turns into a relative one
#   Hi128                        lam = s - floor(s) loses 7 bits at s ~ 127
#   fourier wide                 sin(p) at p ~ 1e3: the fp32 phase is exact to ~ 1e-4
# (the offset, eps, const, spread, dominant and saturated data of the other cases stay a factor 4 below BAR_A in plain fp32.)
FALLBACK = {
    "bn": ("M524800-C4-train-offset",),
    "bilinear": ("Hi128-300x3-T", "Hi128-300x3-F"),
    "fourier": ("wide-D16", "wide-D300"),
    "mha": ("Lq63-Lk64-D16-x6", "Lq65-Lk63-D64-x6", "Lq130-Lk130-D32-x6", "packed-L65-D32-x6"),
}

OPS = tuple(CASES)
ATT_LD = 32          # channel count of the SpatialAtt map tensor: channel 0 of a conv output padded to 32 channels


def case_id(case):
    return case[0]


def ids(op):
    return [case_id(c) for c in CASES[op]]


def by_id(op, name):
    return next(c for c in CASES[op] if c[0] == name)


def is_fallback(op, case):
    return case[0] in FALLBACK.get(op, ())


def _gen(op, case):
    return torch.Generator().manual_seed(zlib.crc32(f"{op}/{case[0]}".encode()))


def _normal_data(gen, shape, kind, eps, plain=(2.0, 0.3)):
    std, mean = {"plain": plain, "eps": (math.sqrt(eps), 0.3 * math.sqrt(eps)), "const": (math.sqrt(eps), 0.3 * math.sqrt(eps)),
                 "offset": (2.0, 30.0)}[kind]
    return torch.randn(*shape, generator=gen) * std + mean


@functools.lru_cache(maxsize=4)
def make(op, case):
    """The CPU fp32 tensors of a case, NHWC.  Shared between tests: do not modify."""
    gen = _gen(op, case)
    rn = lambda *s: torch.randn(*s, generator=gen)
    ru = lambda *s: torch.rand(*s, generator=gen) * 2 - 1
    if op == "ws":
        _, O, ci, k, kind = case
        w = _normal_data(gen, (O, ci, k, k), kind, 9e-6, plain=(0.3, 0.05))          # eps data: weight scale 3e-3
        if kind == "offset":
            w = w * 0.01                                                             # |mean| / std = 15 at a weight's size
        if kind == "const":
            w[0] = 0.75
        return dict(w=w, dy=rn(O, ci, k, k))
    if op == "ln":
        _, M, C, kind = case
        x = _normal_data(gen, (1, M, 1, C), kind, 9e-6)
        if kind == "const":
            x[0, 0] = 0.75
        return dict(x=x, g=1.0 + 0.2 * ru(C), dy=rn(1, M, 1, C))
    if op == "bn":
        _, M, C, kind, training = case
        x = _normal_data(gen, (1, M, 1, C), kind, BN_EPS)
        if kind == "const":
            x[..., 0] = 0.75
        var = {"plain": 4.0, "eps": BN_EPS, "const": BN_EPS, "offset": 4.0}[kind]
        mean = {"plain": 0.3, "offset": 30.0}.get(kind, 0.3 * math.sqrt(BN_EPS))
        return dict(x=x, gamma=1.0 + 0.2 * ru(C), beta=0.1 * ru(C), run_mean=mean * (1 + 0.1 * ru(C)), run_var=var * (1 + 0.3 * ru(C)),
                    dy=rn(1, M, 1, C))
    if op == "bilinear":
        _, B, Hi, Wi, Ho, Wo, C, align, into = case
        d = dict(x=rn(B, Hi, Wi, C), dy=rn(B, Ho, Wo, C))
        if into is not None:
            d["buf"] = rn(B, Ho, Wo, into[1])            # what the destination holds before, and the gradient of all of it
            d["dbuf"] = rn(B, Ho, Wo, into[1])
            d["dy"] = d["dbuf"][..., into[0]:into[0] + C].contiguous()
        return d
    if op == "act":
        _, shape, kind, p = case
        return dict(x=3.0 * rn(*shape), dy=rn(*shape), keep_host=(torch.rand(*shape, generator=gen) >= p).float() / (1.0 - p))
    if op == "fourier":
        _, B, D, kind = case
        if kind == "wide":
            return dict(x=torch.linspace(math.log(1e-4), 0.0, B), W=16.0 * rn(D))
        return dict(x=torch.rand(B, generator=gen), W=(0.5 if kind == "mid" else 0.1) * rn(D))
    if op == "col2im":
        _, B, Hin, Win, C, ks, stride, pad = case
        Ho, Wo = (Hin + 2 * pad - ks) // stride + 1, (Win + 2 * pad - ks) // stride + 1
        return dict(col=rn(B, Ho, Wo, ks * ks, C))
    if op == "mha":
        _, B, Lq, Lk, H, D, scale, kind, packed = case
        C = H * D
        q, k, v, do = rn(B, Lq, C), rn(B, Lk, C), rn(B, Lk, C), rn(B, Lq, C)
        if kind == "x6":
            q, k, v = 6.0 * q, 6.0 * k, 6.0 * v
        elif kind == "soft":
            q, k = 0.5 * q, 0.5 * k
        elif kind == "equal":
            k = k[:, :1].expand(B, Lk, C).contiguous()
        elif kind == "dominant":
            # channel 0 of every head: q = 3, key 7 at 4, the others 0 -> its logit is 12 above a field of spread 0.3 sqrt(D)
            q = q.reshape(B, Lq, H, D).clone(); k = 0.3 * k.reshape(B, Lk, H, D)
            q[..., 0] = 3.0; k[..., 0] = 0.0; k[:, 7, :, 0] = 4.0
            q, k = q.reshape(B, Lq, C), k.reshape(B, Lk, C)
        else:
            assert kind == "plain"
        if packed:
            assert Lq == Lk
            return dict(qkv=torch.cat([q, k, v], dim=-1).contiguous(), dout=do)
        return dict(q=q, k=k, v=v, dout=do)
    if op == "la":
        _, B, N, kind = case
        qkv = 1.5 * rn(B, N, 384)
        if kind == "spread":
            ramp = torch.linspace(-1.0, 1.0, N).reshape(1, N, 1) if N > 1 else torch.zeros(1, 1, 1)
            qkv[:, :, 128:256] = 30.0 * (0.6 * ramp * ru(1, 1, 128).sign() + 0.4 * ru(B, N, 128))   # maxima at either end of the map
        return dict(qkv=qkv, dout=rn(B, N, 128))
    if op == "spatt":
        _, B, H, W, C, qk, att_scale = case
        return dict(att=att_scale * rn(B, H, W, ATT_LD), qk=torch.tensor(qk), h=rn(B, H, W, C), xres=rn(B, H, W, C), dy=rn(B, H, W, C))
    raise KeyError(op)


def reference(op, case, data, device="cpu", keep=None, backward=True):
    """The fp64ref dict of a case, computed on `device`.  keep: the dropout mask / (1 - p) of an `act` case (default: the host-side
    mask of make(), for the CPU tests)."""
    d = {k: v.to(device) for k, v in data.items()}
    dy = lambda n="dy": d[n] if backward else None
    if op == "ws":
        return fp64ref.weight_std(d["w"], WS_EPS, dy())
    if op == "ln":
        return fp64ref.layer_norm_c(d["x"], d["g"], LN_EPS, dy())
    if op == "bn":
        return fp64ref.batch_norm(d["x"], d["gamma"], d["beta"], d["run_mean"], d["run_var"], training=case[4], momentum=BN_MOMENTUM,
                                  eps=BN_EPS, dy=dy())
    if op == "bilinear":
        return fp64ref.bilinear(d["x"], case[4], case[5], case[7], dy())
    if op == "act":
        return fp64ref.act(d["x"], case[2], d["keep_host"] if keep is None else keep, dy())
    if op == "fourier":
        return fp64ref.fourier_features(d["x"], d["W"])
    if op == "col2im":
        return fp64ref.col2im(d["col"], case[1], case[2], case[3], case[5], case[6], case[7])
    if op == "mha":
        if case[8]:
            return fp64ref.mha_packed(d["qkv"], case[4], case[6], dy("dout"))
        return fp64ref.mha(d["q"], d["k"], d["v"], case[4], case[6], dy("dout"))
    if op == "la":
        return fp64ref.linear_attention(d["qkv"], dy("dout"))
    if op == "spatt":
        return fp64ref.spatial_att_gate(d["att"], d["qk"], d["h"], d["xres"], dy())
    raise KeyError(op)


# ------------------------------------------------------------------------------------------------ fp32 torch compositions
DEFECTS = {
    "ws": ("eps dropped", "eps 1e-3", "unbiased variance"),
    "ln": ("eps dropped", "eps 1e-3", "unbiased variance"),
    "bn": ("eps dropped", "unbiased variance", "biased running variance"),
    "bilinear": ("wrong align_corners",),
    "la": ("missing 1/N", "key softmax over the wrong axis"),
    "mha": ("scale applied twice", "lse without the running max"),
    "spatt": ("softsign derivative without the square",),
}


class _Softsign(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, squared):
        ctx.save_for_backward(a)
        ctx.squared = squared
        return a / (1 + a.abs())

    @staticmethod
    def backward(ctx, g):
        (a,) = ctx.saved_tensors
        d = 1 + a.abs()
        return g / (d * d if ctx.squared else d), None


def _grads(outs, wrt, dy, names):
    g = torch.autograd.grad(outs, wrt, dy)
    return dict(zip(names, g))


def torch32(op, case, data, defect=None, keep=None):
    """The outputs of reference() from plain torch on the CPU in the data's own precision (fp32 as make() gives it: the comparator;
    converted to fp64: an independent formulation of the reference), gradients by autograd.  defect: one of DEFECTS[op]."""
    assert defect is None or defect in DEFECTS[op], (op, defect)
    d = {k: v.detach().clone() for k, v in data.items()}
    leaf = lambda n: d[n].requires_grad_(True)
    if op in ("ws", "ln"):
        eps = {"eps dropped": 0.0, "eps 1e-3": 1e-3}.get(defect, WS_EPS if op == "ws" else LN_EPS)
        unb = defect == "unbiased variance"
        if op == "ws":
            w = leaf("w")
            r = w.reshape(w.shape[0], -1)
            y = ((r - r.mean(1, keepdim=True)) * torch.rsqrt(r.var(1, unbiased=unb, keepdim=True) + eps)).reshape(w.shape)
            return dict(y=y.detach(), **_grads(y, [w], d["dy"], ["dw"]))
        x, g = leaf("x"), leaf("g")
        y = (x - x.mean(-1, keepdim=True)) * torch.rsqrt(x.var(-1, unbiased=unb and x.shape[-1] > 1, keepdim=True) + eps) * g
        return dict(y=y.detach(), **_grads(y, [x, g], d["dy"], ["dx", "dg"]))
    if op == "bn":
        _, M, C, kind, training = case
        x, gamma, beta = leaf("x"), leaf("gamma"), leaf("beta")
        rm, rv = d["run_mean"], d["run_var"]
        r = x.reshape(M, C)
        if defect is None:
            y = F.batch_norm(r, rm, rv, gamma, beta, training, BN_MOMENTUM, BN_EPS)
        else:
            eps = 0.0 if defect == "eps dropped" else BN_EPS
            if training:
                mean, vb = r.mean(0), r.var(0, unbiased=False)
                vu = vb * (M / max(M - 1, 1))
                with torch.no_grad():
                    rm.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * mean)
                    rv.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * (vb if defect == "biased running variance" else vu))
                var = vu if defect == "unbiased variance" else vb
            else:
                mean, var = rm, rv
            y = (r - mean) * torch.rsqrt(var + eps) * gamma + beta
        y = y.reshape(x.shape)
        return dict(y=y.detach(), running_mean=rm, running_var=rv, **_grads(y, [x, gamma, beta], d["dy"], ["dx", "dgamma", "dbeta"]))
    if op == "bilinear":
        _, B, Hi, Wi, Ho, Wo, C, align, into = case
        x = leaf("x")
        if defect:
            align = not align
        y = F.interpolate(x.permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=align).permute(0, 2, 3, 1)
        return dict(y=y.detach(), **_grads(y, [x], d["dy"], ["dx"]))
    if op == "act":
        _, shape, kind, p = case
        x = leaf("x")
        y = {"relu": F.relu, "gelu": F.gelu, "id": lambda t: t * 1.0}[kind](x) * (d["keep_host"] if keep is None else keep.to(d["x"].dtype).cpu())
        return dict(y=y.detach(), **_grads(y, [x], d["dy"], ["dx"]))
    if op == "fourier":
        p = d["x"][:, None] * d["W"][None, :] * 2 * math.pi
        return dict(y=torch.cat([torch.sin(p), torch.cos(p)], dim=-1))
    if op == "col2im":
        _, B, Hin, Win, C, ks, stride, pad = case
        col = d["col"]
        Ho, Wo = col.shape[1], col.shape[2]
        cols = col.reshape(B, Ho * Wo, ks * ks, C).permute(0, 3, 2, 1).reshape(B, C * ks * ks, Ho * Wo)
        return dict(dx=F.fold(cols, (Hin, Win), ks, padding=pad, stride=stride).permute(0, 2, 3, 1))
    if op == "mha":
        _, B, Lq, Lk, H, D, scale, kind, packed = case
        C = H * D
        if packed:
            qkv = leaf("qkv")
            q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        else:
            q, k, v = leaf("q"), leaf("k"), leaf("v")
        hd = lambda t, L: t.reshape(B, L, H, D).permute(0, 2, 1, 3)
        s = (hd(q, Lq) * scale) @ hd(k, Lk).transpose(-1, -2)
        if defect == "scale applied twice":
            s = s * scale
        if defect == "lse without the running max":
            e = torch.exp(s)
            P = e / e.sum(-1, keepdim=True)
        else:
            P = s.softmax(-1)
        o = (P @ hd(v, Lk)).permute(0, 2, 1, 3).reshape(B, Lq, C)
        if packed:
            return dict(out=o.detach(), **_grads(o, [qkv], d["dout"], ["dqkv"]))
        return dict(out=o.detach(), **_grads(o, [q, k, v], d["dout"], ["dq", "dk", "dv"]))
    if op == "la":
        _, B, N, kind = case
        qkv = leaf("qkv")
        q, k, v = qkv.reshape(B, N, 3, 4, 32).unbind(2)                               # [B][N][4][32]
        ks = k.softmax(dim=-1 if defect == "key softmax over the wrong axis" else 1)
        ctx = torch.einsum("bnhd,bnhe->bhde", ks, v if defect == "missing 1/N" else v / N)
        o = torch.einsum("bhde,bnhd->bnhe", ctx, q.softmax(-1) * 32 ** -0.5).reshape(B, N, 128)
        return dict(out=o.detach(), **_grads(o, [qkv], d["dout"], ["dqkv"]))
    if op == "spatt":
        _, B, H, W, C, _, _ = case
        att, qk, h = leaf("att"), leaf("qk"), leaf("h")
        a = att.reshape(B, H * W, ATT_LD)[:, :, 0]
        q, k = qk[0] * a + qk[1], qk[2] * a + qk[3]
        av = ((q[:, :, None] * k[:, None, :]).softmax(-1) @ a[:, :, None])[:, :, 0]
        y = _Softsign.apply(av, defect is None)[:, :, None] * h.reshape(B, H * W, C) + d["xres"].reshape(B, H * W, C)
        y = y.reshape(h.shape)
        return dict(y=y.detach(), **_grads(y, [h, att, qk], d["dy"], ["dh", "datt", "dqk"]))
    raise KeyError(op)
