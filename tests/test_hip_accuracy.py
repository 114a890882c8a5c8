"""GPU: every conv / attention launch plan the shipped configs reach, against fp64.

Which kernel runs, with which split-K count and which workgroup form, depends on the batch: the 96- and 128-cout forms of the fp16
split format and the unsplit weight gradients are only taken at production sizes.  This file

1. records, through a wrapper of ops.call, every launch of the conv / GEMM / attention kernels in one training step and one sampling
   pass of each shipped config (bench.build_model), with the default switches and with ADM_DETERMINISTIC, and asserts that every
   launch is in PRODUCTION_LAUNCHES below (a dispatch or shape change fails here until the sweep covers it);
2. drives ops.conv2d / ops.attention at every geometry of that table, asserts that the recorded launches come back, and checks
   forward, data gradient and weight gradient against the fp64 reference of tests/fp64ref.py with the bars below.

A launch is keyed by (symbol, its integer arguments, which of its pointer arguments are null): the integers hold the geometry, the
split-K workspace size or split count, and the flags.  The table maps the op-level SITE of a launch (which entry point, at which
geometry, with which bounds and gradient sinks) to the keys it produced, so the sweep can rebuild the call.

Bars, per output and relative to the same contraction on |operands| (fp64ref.errors):
  A (every path):       e_max <= BAR_A
  B (split formats vs the f32-MFMA kernel on the same data):
                        e_rms <= 2 e_rms(f32) + 1e-9,   e_max <= max(2 e_max(f32), 4e-7)
"""
import ctypes
import os
import re
import sys

import pytest
import torch

from oracle import fill

import fp64ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BAR_A = 1e-5

CONFIGS = {"cifar": (128, 32), "latent": (32, 64), "latent-ae": (32, 256), "sr": (16, 512)}     # batch, image side

_RECORDED = re.compile(r"^adm_(conv_fwd|conv_wgrad|gemm_x6|gemm_wgrad_x6|attn_)")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from adm_amd import hip, ops as _ops
    hip.lib()        # raises if the HIP library is missing: no fallback
    return _ops


# ------------------------------------------------------------------------------------------------ the launch recorder
def launch_key(name, args):
    """(symbol, integer arguments, pointer arguments as 'p' / '0' for null)."""
    ints = tuple(int(a) for a in args if isinstance(a, int) and not isinstance(a, bool))
    ptrs = "".join("0" if a is None or (isinstance(a, ctypes.c_void_p) and not a.value) else "p"
                   for a in args if a is None or isinstance(a, ctypes.c_void_p))
    return (name, ints, ptrs)


class Recorder:
    """Forwards every ops.call (and ops_cond.call) and records {site: {key}} for the symbols of _RECORDED.  The site is set by wrappers
    of the op-level entry points (conv, strided / generic conv, matmul_nt, attention; forward and backward)."""

    def __init__(self, mp):
        from adm_amd import ops, ops_cond
        self.launches = {}
        self.site = None
        rec = self

        def wrap_call(orig):
            def call(name, *args):
                if _RECORDED.match(name):
                    rec.launches.setdefault(rec.site, set()).add(launch_key(name, args))
                return orig(name, *args)
            return call

        mp.setattr(ops, "call", wrap_call(ops.call))
        mp.setattr(ops_cond, "call", wrap_call(ops_cond.call))

        def enter(site_of, orig, static):
            def fn(*a, **k):
                prev, rec.site = rec.site, site_of(*a, **k)
                try:
                    return orig(*a, **k)
                finally:
                    rec.site = prev
            return staticmethod(fn) if static else fn

        def nb(t):
            return t is not None

        def conv_fwd(ctx, x, weight, bias, residual, ks, up, qkv, tile, amax=None):
            B, H, W, _ = x.shape
            ctx._census = ("conv", B, H, W, weight.shape[1], weight.shape[0], ks, int(up), nb(bias), nb(residual), nb(amax),
                           ops._SELECT_BATCH)
            return ctx._census

        def conv_bwd(ctx, dy):
            x, weight, bias = ctx.saved_tensors
            ni = ctx.needs_input_grad
            bound = dy.is_contiguous() and ops._get_amax(dy) is not None
            return (("conv-bwd",) + ctx._census[1:]
                    + (bound, ops.DETERMINISTIC, ni[0], ni[1], ni[2] and bias is not None,
                       ops._direct_grad(weight) is not None, ops._direct_grad(bias) is not None))

        def gen_fwd(ctx, x, weight, bias, stride, pad):
            B, H, W, _ = x.shape
            ctx._census = ("generic", B, H, W, weight.shape[1], weight.shape[0], weight.shape[-1], stride, pad, nb(bias))
            return ctx._census

        def gen_bwd(ctx, dy):
            ni = ctx.needs_input_grad
            return ("generic-bwd",) + ctx._census[1:] + (ni[0], ni[1], ni[2] and ctx.saved_tensors[2] is not None)

        def strided(x, weight, bias=None, *, stride=2, pad_lo=0, pad_hi=1):
            B, H, W, _ = x.shape
            return ("strided", B, H, W, weight.shape[1], weight.shape[0], weight.shape[-1], stride, pad_lo, pad_hi, nb(bias))

        def mm(a, b, bias=None, out=None):
            return ("mm", a.shape[0], b.shape[0], a.shape[1], nb(bias))

        def attn_fwd(ctx, qkv, heads, amax=None):
            B, H, W, _ = qkv.shape
            ctx._census = ("attn", B, H * W, heads, nb(amax))
            return ctx._census

        def attn_bwd(ctx, dout):
            bound = dout.is_contiguous() and ops._get_amax(dout) is not None
            return ("attn-bwd",) + ctx._census[1:] + (bound,)

        def affine_fwd(ctx, emb, grp, *params):
            ctx._census = ("affine-group", emb.shape[0], emb.shape[1], grp.total)
            return ctx._census

        def affine_bwd(ctx, *grads):
            return ("affine-group-bwd",) + ctx._census[1:]

        for cls, name, site_of in ((ops._AffineGroupFn, "forward", affine_fwd), (ops._AffineGroupFn, "backward", affine_bwd),
                                   (ops._Conv, "forward", conv_fwd), (ops._Conv, "backward", conv_bwd),
                                   (ops_cond._ConvGeneric, "forward", gen_fwd), (ops_cond._ConvGeneric, "backward", gen_bwd),
                                   (ops._Attention, "forward", attn_fwd), (ops._Attention, "backward", attn_bwd)):
            mp.setattr(cls, name, enter(site_of, getattr(cls, name), True))
        mp.setattr(ops, "conv2d_strided", enter(strided, ops.conv2d_strided, False))
        mp.setattr(ops, "matmul_nt", enter(mm, ops.matmul_nt, False))

    def pairs(self):
        return {(s, k) for s, ks in self.launches.items() for k in ks}


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def census(config, det):
    """{(site, key)} of one training step (forward + backward, gradients into the flat buffer as bench.py runs them) and one
    2-step sample() (the no-grad forward, and the autoencoder decode where there is one) of a shipped config."""
    from adm_amd import ops
    from adm_amd.optim import FlatParams
    B, R = CONFIGS[config]
    gpu = torch.device("cuda:0")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "DETERMINISTIC", det)
        mp.setattr(ops, "PROFILE", None)
        dpm = _bench().build_model(gpu, config=config).train()
        flat = FlatParams(dpm)
        g = torch.Generator(device=gpu).manual_seed(100)
        batch = {"image": torch.rand(B, 3, R, R, device=gpu, generator=g) * 2 - 1}
        if config == "sr":       # bench.py's synthetic condition pyramid (Swin-B geometry of a 128x128 low-resolution image)
            batch["cond"] = [torch.randn(B, 128 << i, 32 >> i, 32 >> i, device=gpu, generator=g) for i in range(4)]
        rec = Recorder(mp)
        flat.zero_grad()
        loss, _ = dpm.training_step(batch)
        loss.backward()
        ops.flush_deferred_unpack()
        dpm.eval()
        dpm.sampling_timesteps = 2
        with torch.no_grad():
            img = dpm.sample(batch_size=B, **({"cond": batch["cond"]} if config == "sr" else {}))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss)), (config, float(loss))
        assert bool(torch.isfinite(img).all()), (config, int((~torch.isfinite(img)).sum()))
        return rec.pairs()


# ------------------------------------------------------------------------------------------------ the table
PRODUCTION_LAUNCHES = {      # written from the census above; site -> launch keys
    ('affine-group', 1, 512, 16384): (('adm_conv_fwd', (1, 1, 1, 512, 512, 16384, 16384, 16384, 16384, 1, 0, -1), 'ppp0p'),),
    ('affine-group', 1, 768, 39168): (('adm_conv_fwd', (1, 1, 1, 768, 768, 39168, 39168, 39168, 39168, 1, 0, -1), 'ppp0p'),),
    ('affine-group', 32, 512, 16384): (('adm_conv_fwd', (32, 1, 1, 512, 512, 16384, 16384, 16384, 16384, 1, 0, -1), 'ppp0p'),),
    ('affine-group', 128, 768, 39168): (('adm_conv_fwd', (128, 1, 1, 768, 768, 39168, 39168, 39168, 39168, 1, 0, -1), 'ppp0p'),),
    ('affine-group-bwd', 32, 512, 16384): (('adm_conv_fwd_ws', (524288, 32, 1, 1, 16384, 16384, 512, 512, 512, 512, 1, 0), 'pp00pp'), ('adm_conv_wgrad_bias', (32, 1, 1, 512, 512, 16384, 16384, 1, 0, -1), 'pppp')),
    ('affine-group-bwd', 128, 768, 39168): (('adm_conv_fwd_ws', (3145728, 128, 1, 1, 39168, 39168, 768, 768, 768, 768, 1, 0), 'pp00pp'), ('adm_conv_wgrad_bias', (128, 1, 1, 768, 768, 39168, 39168, 1, 0, -1), 'pppp')),
    ('attn', 32, 64, 4, True): (('adm_attn_fwd_h3', (32, 64, 4), 'pppp'),),
    ('attn', 32, 256, 4, True): (('adm_attn_fwd_h3', (32, 256, 4), 'pppp'),),
    ('attn', 128, 16, 6, True): (('adm_attn_fwd', (128, 16, 6), 'ppp'),),
    ('attn', 128, 64, 6, True): (('adm_attn_fwd_h3', (128, 64, 6), 'pppp'),),
    ('attn', 128, 256, 6, True): (('adm_attn_fwd_h3', (128, 256, 6), 'pppp'),),
    ('attn-bwd', 32, 64, 4, True, True): (('adm_attn_bwd_h3', (32, 64, 4), 'ppppppppp'),),
    ('attn-bwd', 32, 256, 4, True, True): (('adm_attn_bwd_h3', (32, 256, 4), 'ppppppppp'),),
    ('attn-bwd', 128, 16, 6, True, True): (('adm_attn_bwd_amax', (128, 16, 6), 'ppppppp'),),
    ('attn-bwd', 128, 64, 6, True, True): (('adm_attn_bwd_h3', (128, 64, 6), 'ppppppppp'),),
    ('attn-bwd', 128, 256, 6, True, True): (('adm_attn_bwd_h3', (128, 256, 6), 'ppppppppp'),),
    ('conv', 1, 1, 1, 128, 512, 1, 0, True, False, False, None): (('adm_conv_fwd', (1, 1, 1, 128, 128, 512, 512, 512, 512, 1, 0, -1), 'ppp0p'),),
    ('conv', 1, 1, 1, 192, 768, 1, 0, True, False, False, None): (('adm_conv_fwd', (1, 1, 1, 192, 192, 768, 768, 768, 768, 1, 0, -1), 'ppp0p'),),
    ('conv', 1, 1, 1, 512, 256, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (512, 1, 1, 1, 512, 512, 256, 256, 256, 256, 1, 0), 'ppp0pp'),),
    ('conv', 1, 1, 1, 512, 512, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (1024, 1, 1, 1, 512, 512, 512, 512, 512, 512, 1, 0), 'ppp0pp'),),
    ('conv', 1, 1, 1, 768, 384, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (1152, 1, 1, 1, 768, 768, 384, 384, 384, 384, 1, 0), 'ppp0pp'),),
    ('conv', 1, 1, 1, 768, 768, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (2304, 1, 1, 1, 768, 768, 768, 768, 768, 768, 1, 0), 'ppp0pp'),),
    ('conv', 2, 128, 128, 3, 3, 1, 0, True, False, True, 16): (('adm_conv_fwd', (2, 128, 128, 32, 32, 32, 32, 32, 32, 1, 0, -1), 'ppp0p'),),
    ('conv', 2, 128, 128, 3, 512, 3, 0, True, False, False, 16): (('adm_conv_fwd_wino2d_x6', (0, 2, 128, 128, 32, 32, 512, 512, 512, 512), 'ppp0p0'),),
    ('conv', 2, 128, 128, 6, 6, 1, 0, True, False, False, 16): (('adm_conv_fwd', (2, 128, 128, 32, 32, 32, 32, 32, 32, 1, 0, -1), 'ppp0p'),),
    ('conv', 2, 128, 128, 256, 512, 1, 0, True, False, False, 16): (('adm_gemm_x6_amax', (32768, 256, 256, 512, 512, 512, 512), 'ppp0pp'),),
    ('conv', 2, 128, 128, 256, 512, 3, 0, True, False, False, 16): (('adm_conv_fwd_wino2d_x6', (0, 2, 128, 128, 256, 256, 512, 512, 512, 512), 'ppp0p0'),),
    ('conv', 2, 128, 128, 512, 6, 3, 0, True, False, False, 16): (('adm_conv_fwd_wino2d_x6', (0, 2, 128, 128, 512, 512, 32, 32, 32, 32), 'ppp0p0'),),
    ('conv', 2, 128, 128, 512, 512, 1, 0, True, False, False, 16): (('adm_gemm_x6_amax', (32768, 512, 512, 512, 512, 512, 512), 'ppp0pp'),),
    ('conv', 2, 128, 128, 512, 512, 1, 0, True, True, False, 16): (('adm_gemm_x6_amax', (32768, 512, 512, 512, 512, 512, 512), 'pppppp'),),
    ('conv', 2, 128, 128, 512, 512, 3, 0, True, False, False, 16): (('adm_conv_fwd_wino2d_x6', (0, 2, 128, 128, 512, 512, 512, 512, 512, 512), 'ppp0p0'),),
    ('conv', 2, 128, 128, 512, 512, 3, 0, True, True, False, 16): (('adm_conv_fwd_wino2d_x6', (0, 2, 128, 128, 512, 512, 512, 512, 512, 512), 'ppppp0'),),
    ('conv', 2, 128, 128, 512, 512, 3, 1, True, False, False, 16): (('adm_conv_fwd_wino2d_x6_up', (0, 2, 256, 256, 512, 512, 512, 512, 512, 512), 'ppp0p0'),),
    ('conv', 2, 256, 256, 128, 256, 1, 0, True, False, False, 16): (('adm_gemm_x6_amax', (131072, 128, 128, 256, 256, 256, 256), 'ppp0pp'),),
    ('conv', 2, 256, 256, 128, 256, 3, 0, True, False, False, 16): (('adm_conv_fwd_wino2d_x6', (0, 2, 256, 256, 128, 128, 256, 256, 256, 256), 'ppp0p0'),),
    ('conv', 2, 256, 256, 256, 256, 3, 0, True, False, False, 16): (('adm_conv_fwd_wino2d_x6', (0, 2, 256, 256, 256, 256, 256, 256, 256, 256), 'ppp0p0'),),
    ('conv', 2, 256, 256, 256, 256, 3, 0, True, True, False, 16): (('adm_conv_fwd_wino2d_x6', (0, 2, 256, 256, 256, 256, 256, 256, 256, 256), 'ppppp0'),),
    ('conv', 2, 256, 256, 256, 256, 3, 1, True, False, False, 16): (('adm_conv_fwd_wino2d_x6_up', (0, 2, 512, 512, 256, 256, 256, 256, 256, 256), 'ppp0p0'),),
    ('conv', 2, 256, 256, 512, 256, 1, 0, True, False, False, 16): (('adm_gemm_x6_amax', (131072, 512, 512, 256, 256, 256, 256), 'ppp0pp'),),
    ('conv', 2, 256, 256, 512, 256, 3, 0, True, False, False, 16): (('adm_conv_fwd_wino2d_x6', (0, 2, 256, 256, 512, 512, 256, 256, 256, 256), 'ppp0p0'),),
    ('conv', 2, 512, 512, 3, 128, 3, 0, True, False, True, 16): (('adm_conv_fwd_wino2d_h3', (0, 2, 512, 512, 32, 32, 128, 128, 128, 128, 0), 'ppp0p0p'),),
    ('conv', 2, 512, 512, 128, 3, 3, 0, True, False, False, 16): (('adm_conv_fwd_wino2d_x6', (0, 2, 512, 512, 128, 128, 32, 32, 32, 32), 'ppp0p0'),),
    ('conv', 2, 512, 512, 128, 128, 3, 0, True, False, False, 16): (('adm_conv_fwd_wino2d_x6', (0, 2, 512, 512, 128, 128, 128, 128, 128, 128), 'ppp0p0'),),
    ('conv', 2, 512, 512, 128, 128, 3, 0, True, True, False, 16): (('adm_conv_fwd_wino2d_x6', (0, 2, 512, 512, 128, 128, 128, 128, 128, 128), 'ppppp0'),),
    ('conv', 2, 512, 512, 256, 128, 1, 0, True, False, False, 16): (('adm_gemm_x6_amax', (524288, 256, 256, 128, 128, 128, 128), 'ppp0pp'),),
    ('conv', 2, 512, 512, 256, 128, 3, 0, True, False, False, 16): (('adm_conv_fwd_wino2d_x6', (0, 2, 512, 512, 256, 256, 128, 128, 128, 128), 'ppp0p0'),),
    ('conv', 8, 64, 64, 3, 3, 1, 0, True, False, True, 32): (('adm_conv_fwd', (8, 64, 64, 32, 32, 32, 32, 32, 32, 1, 0, -1), 'ppp0p'),),
    ('conv', 8, 64, 64, 3, 512, 3, 0, True, False, False, 32): (('adm_conv_fwd_wino2d_x6', (0, 8, 64, 64, 32, 32, 512, 512, 512, 512), 'ppp0p0'),),
    ('conv', 8, 64, 64, 6, 6, 1, 0, True, False, False, 32): (('adm_conv_fwd', (8, 64, 64, 32, 32, 32, 32, 32, 32, 1, 0, -1), 'ppp0p'),),
    ('conv', 8, 64, 64, 256, 512, 1, 0, True, False, False, 32): (('adm_gemm_x6_amax', (32768, 256, 256, 512, 512, 512, 512), 'ppp0pp'),),
    ('conv', 8, 64, 64, 256, 512, 3, 0, True, False, False, 32): (('adm_conv_fwd_wino2d_x6', (0, 8, 64, 64, 256, 256, 512, 512, 512, 512), 'ppp0p0'),),
    ('conv', 8, 64, 64, 512, 6, 3, 0, True, False, False, 32): (('adm_conv_fwd_wino2d_x6', (0, 8, 64, 64, 512, 512, 32, 32, 32, 32), 'ppp0p0'),),
    ('conv', 8, 64, 64, 512, 512, 1, 0, True, False, False, 32): (('adm_gemm_x6_amax', (32768, 512, 512, 512, 512, 512, 512), 'ppp0pp'),),
    ('conv', 8, 64, 64, 512, 512, 1, 0, True, True, False, 32): (('adm_gemm_x6_amax', (32768, 512, 512, 512, 512, 512, 512), 'pppppp'),),
    ('conv', 8, 64, 64, 512, 512, 3, 0, True, False, False, 32): (('adm_conv_fwd_wino2d_x6', (0, 8, 64, 64, 512, 512, 512, 512, 512, 512), 'ppp0p0'),),
    ('conv', 8, 64, 64, 512, 512, 3, 0, True, True, False, 32): (('adm_conv_fwd_wino2d_x6', (0, 8, 64, 64, 512, 512, 512, 512, 512, 512), 'ppppp0'),),
    ('conv', 8, 64, 64, 512, 512, 3, 1, True, False, False, 32): (('adm_conv_fwd_wino2d_x6_up', (0, 8, 128, 128, 512, 512, 512, 512, 512, 512), 'ppp0p0'),),
    ('conv', 8, 128, 128, 128, 256, 1, 0, True, False, False, 32): (('adm_gemm_x6_amax', (131072, 128, 128, 256, 256, 256, 256), 'ppp0pp'),),
    ('conv', 8, 128, 128, 128, 256, 3, 0, True, False, False, 32): (('adm_conv_fwd_wino2d_x6', (0, 8, 128, 128, 128, 128, 256, 256, 256, 256), 'ppp0p0'),),
    ('conv', 8, 128, 128, 256, 256, 3, 0, True, False, False, 32): (('adm_conv_fwd_wino2d_x6', (0, 8, 128, 128, 256, 256, 256, 256, 256, 256), 'ppp0p0'),),
    ('conv', 8, 128, 128, 256, 256, 3, 0, True, True, False, 32): (('adm_conv_fwd_wino2d_x6', (0, 8, 128, 128, 256, 256, 256, 256, 256, 256), 'ppppp0'),),
    ('conv', 8, 128, 128, 256, 256, 3, 1, True, False, False, 32): (('adm_conv_fwd_wino2d_x6_up', (0, 8, 256, 256, 256, 256, 256, 256, 256, 256), 'ppp0p0'),),
    ('conv', 8, 128, 128, 512, 256, 1, 0, True, False, False, 32): (('adm_gemm_x6_amax', (131072, 512, 512, 256, 256, 256, 256), 'ppp0pp'),),
    ('conv', 8, 128, 128, 512, 256, 3, 0, True, False, False, 32): (('adm_conv_fwd_wino2d_x6', (0, 8, 128, 128, 512, 512, 256, 256, 256, 256), 'ppp0p0'),),
    ('conv', 8, 256, 256, 3, 128, 3, 0, True, False, True, 32): (('adm_conv_fwd_wino2d_h3', (0, 8, 256, 256, 32, 32, 128, 128, 128, 128, 0), 'ppp0p0p'),),
    ('conv', 8, 256, 256, 128, 3, 3, 0, True, False, False, 32): (('adm_conv_fwd_wino2d_x6', (0, 8, 256, 256, 128, 128, 32, 32, 32, 32), 'ppp0p0'),),
    ('conv', 8, 256, 256, 128, 128, 3, 0, True, False, False, 32): (('adm_conv_fwd_wino2d_x6', (0, 8, 256, 256, 128, 128, 128, 128, 128, 128), 'ppp0p0'),),
    ('conv', 8, 256, 256, 128, 128, 3, 0, True, True, False, 32): (('adm_conv_fwd_wino2d_x6', (0, 8, 256, 256, 128, 128, 128, 128, 128, 128), 'ppppp0'),),
    ('conv', 8, 256, 256, 256, 128, 1, 0, True, False, False, 32): (('adm_gemm_x6_amax', (524288, 256, 256, 128, 128, 128, 128), 'ppp0pp'),),
    ('conv', 8, 256, 256, 256, 128, 3, 0, True, False, False, 32): (('adm_conv_fwd_wino2d_x6', (0, 8, 256, 256, 256, 256, 128, 128, 128, 128), 'ppp0p0'),),
    ('conv', 16, 1, 1, 128, 512, 1, 0, True, False, False, None): (('adm_conv_fwd', (16, 1, 1, 128, 128, 512, 512, 512, 512, 1, 0, -1), 'ppp0p'),),
    ('conv', 16, 1, 1, 512, 256, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (8192, 16, 1, 1, 512, 512, 256, 256, 256, 256, 1, 0), 'ppp0pp'),),
    ('conv', 16, 1, 1, 512, 512, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (16384, 16, 1, 1, 512, 512, 512, 512, 512, 512, 1, 0), 'ppp0pp'),),
    ('conv', 16, 1, 1, 512, 1024, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (32768, 16, 1, 1, 512, 512, 1024, 1024, 1024, 1024, 1, 0), 'ppp0pp'),),
    ('conv', 16, 4, 4, 128, 256, 1, 0, True, False, False, None): (('adm_conv_fwd', (16, 4, 4, 128, 128, 256, 256, 256, 256, 1, 0, -1), 'ppp0p'),),
    ('conv', 16, 4, 4, 256, 128, 1, 0, True, False, False, None): (('adm_conv_fwd', (16, 4, 4, 256, 256, 128, 128, 128, 128, 1, 0, -1), 'ppp0p'),),
    ('conv', 16, 4, 4, 256, 512, 1, 0, True, False, False, None): (('adm_conv_fwd', (16, 4, 4, 256, 256, 512, 512, 512, 512, 1, 0, -1), 'ppp0p'),),
    ('conv', 16, 4, 4, 512, 256, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (131072, 16, 4, 4, 512, 512, 256, 256, 256, 256, 1, 0), 'ppp0pp'),),
    ('conv', 16, 4, 4, 512, 512, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (262144, 16, 4, 4, 512, 512, 512, 512, 512, 512, 1, 0), 'ppp0pp'),),
    ('conv', 16, 4, 4, 512, 1024, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (524288, 16, 4, 4, 512, 512, 1024, 1024, 1024, 1024, 1, 0), 'ppp0pp'),),
    ('conv', 16, 4, 4, 1024, 512, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (524288, 16, 4, 4, 1024, 1024, 512, 512, 512, 512, 1, 0), 'ppp0pp'),),
    ('conv', 16, 4, 4, 1024, 512, 1, 0, True, False, True, None): (('adm_conv_fwd_ws', (524288, 16, 4, 4, 1024, 1024, 512, 512, 512, 512, 1, 0), 'ppp0pp'),),
    ('conv', 16, 8, 8, 256, 256, 1, 0, True, False, False, None): (('adm_conv_fwd', (16, 8, 8, 256, 256, 256, 256, 256, 256, 1, 0, -1), 'ppp0p'),),
    ('conv', 16, 8, 8, 256, 512, 1, 0, True, False, False, None): (('adm_conv_fwd', (16, 8, 8, 256, 256, 512, 512, 512, 512, 1, 0, -1), 'ppp0p'),),
    ('conv', 16, 8, 8, 512, 256, 1, 0, True, False, True, None): (('adm_conv_fwd_ws', (524288, 16, 8, 8, 512, 512, 256, 256, 256, 256, 1, 0), 'ppp0pp'),),
    ('conv', 16, 16, 16, 128, 128, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (4096, 128, 128, 128, 128, 128, 128), 'ppp0ppp'),),
    ('conv', 16, 16, 16, 128, 256, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (4096, 128, 128, 256, 256, 256, 256), 'ppp0ppp'),),
    ('conv', 16, 16, 16, 128, 512, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (4096, 128, 128, 512, 512, 512, 512), 'ppp0pp'),),
    ('conv', 16, 16, 16, 128, 512, 1, 0, True, True, False, None): (('adm_gemm_x6_amax', (4096, 128, 128, 512, 512, 512, 512), 'pppppp'),),
    ('conv', 16, 16, 16, 256, 128, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (4096, 256, 256, 128, 128, 128, 128), 'ppp0ppp'),),
    ('conv', 16, 16, 16, 512, 1, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (262144, 16, 16, 16, 512, 512, 32, 32, 32, 32, 1, 0), 'ppp0pp'),),
    ('conv', 16, 16, 16, 512, 384, 1, 0, False, False, False, None): (('adm_gemm_x6_amax', (4096, 512, 512, 384, 384, 384, 384), 'pp00pp'),),
    ('conv', 16, 16, 16, 512, 512, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (4096, 512, 512, 512, 512, 512, 512), 'ppp0pp'),),
    ('conv', 16, 16, 16, 512, 512, 1, 0, True, True, False, None): (('adm_gemm_x6_amax', (4096, 512, 512, 512, 512, 512, 512), 'pppppp'),),
    ('conv', 16, 16, 16, 512, 512, 3, 0, True, False, False, None): (('adm_conv_fwd_wino2d_x6', (4194304, 16, 16, 16, 512, 512, 512, 512, 512, 512), 'ppp0pp'),),
    ('conv', 16, 16, 16, 512, 512, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (4194304, 16, 16, 16, 512, 512, 512, 512, 512, 512, 0), 'ppp0ppp'),),
    ('conv', 16, 16, 16, 512, 512, 3, 1, True, False, False, None): (('adm_conv_fwd_wino2d_x6_up', (0, 16, 32, 32, 512, 512, 512, 512, 512, 512), 'ppp0p0'),),
    ('conv', 16, 16, 16, 1024, 512, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (4096, 1024, 1024, 512, 512, 512, 512), 'ppp0ppp'),),
    ('conv', 16, 16, 16, 1024, 512, 1, 0, True, True, True, None): (('adm_gemm_x6_h3', (4096, 1024, 1024, 512, 512, 512, 512), 'ppppppp'),),
    ('conv', 16, 16, 16, 1024, 512, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (4194304, 16, 16, 16, 1024, 1024, 512, 512, 512, 512, 0), 'ppp0ppp'),),
    ('conv', 16, 32, 32, 128, 128, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (16384, 128, 128, 128, 128, 128, 128), 'ppp0ppp'),),
    ('conv', 16, 32, 32, 128, 256, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (16384, 128, 128, 256, 256, 256, 256), 'ppp0pp'),),
    ('conv', 16, 32, 32, 128, 512, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (16384, 128, 128, 512, 512, 512, 512), 'ppp0pp'),),
    ('conv', 16, 32, 32, 256, 256, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (16384, 256, 256, 256, 256, 256, 256), 'ppp0pp'),),
    ('conv', 16, 32, 32, 256, 256, 1, 0, True, True, False, None): (('adm_gemm_x6_amax', (16384, 256, 256, 256, 256, 256, 256), 'pppppp'),),
    ('conv', 16, 32, 32, 256, 256, 3, 0, True, False, False, None): (('adm_conv_fwd_wino2d_x6', (0, 16, 32, 32, 256, 256, 256, 256, 256, 256), 'ppp0p0'),),
    ('conv', 16, 32, 32, 256, 256, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 16, 32, 32, 256, 256, 256, 256, 256, 256, 0), 'ppp0p0p'),),
    ('conv', 16, 32, 32, 256, 384, 1, 0, False, False, False, None): (('adm_gemm_x6_amax', (16384, 256, 256, 384, 384, 384, 384), 'pp00pp'),),
    ('conv', 16, 32, 32, 512, 256, 1, 0, True, True, True, None): (('adm_gemm_x6_h3', (16384, 512, 512, 256, 256, 256, 256), 'ppppppp'),),
    ('conv', 16, 32, 32, 512, 256, 3, 1, True, False, False, None): (('adm_conv_fwd_wino2d_x6_up', (0, 16, 64, 64, 512, 512, 256, 256, 256, 256), 'ppp0p0'),),
    ('conv', 16, 32, 32, 512, 384, 1, 0, False, False, False, None): (('adm_gemm_x6_amax', (16384, 512, 512, 384, 384, 384, 384), 'pp00pp'),),
    ('conv', 16, 32, 32, 512, 512, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (16384, 512, 512, 512, 512, 512, 512), 'ppp0pp'),),
    ('conv', 16, 32, 32, 512, 512, 1, 0, True, True, False, None): (('adm_gemm_x6_amax', (16384, 512, 512, 512, 512, 512, 512), 'pppppp'),),
    ('conv', 16, 32, 32, 512, 512, 3, 0, True, False, False, None): (('adm_conv_fwd_wino2d_x6', (0, 16, 32, 32, 512, 512, 512, 512, 512, 512), 'ppp0p0'),),
    ('conv', 16, 32, 32, 768, 512, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (16384, 768, 768, 512, 512, 512, 512), 'ppp0ppp'),),
    ('conv', 16, 32, 32, 768, 512, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 16, 32, 32, 768, 768, 512, 512, 512, 512, 0), 'ppp0p0p'),),
    ('conv', 16, 32, 32, 1024, 512, 1, 0, True, True, True, None): (('adm_gemm_x6_h3', (16384, 1024, 1024, 512, 512, 512, 512), 'ppppppp'),),
    ('conv', 16, 64, 64, 128, 128, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (65536, 128, 128, 128, 128, 128, 128), 'ppp0pp'),),
    ('conv', 16, 64, 64, 128, 128, 1, 0, True, True, False, None): (('adm_gemm_x6_amax', (65536, 128, 128, 128, 128, 128, 128), 'pppppp'),),
    ('conv', 16, 64, 64, 128, 128, 3, 0, True, False, False, None): (('adm_conv_fwd_wino2d_x6', (0, 16, 64, 64, 128, 128, 128, 128, 128, 128), 'ppp0p0'),),
    ('conv', 16, 64, 64, 128, 128, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 16, 64, 64, 128, 128, 128, 128, 128, 128, 0), 'ppp0p0p'),),
    ('conv', 16, 64, 64, 128, 256, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (65536, 128, 128, 256, 256, 256, 256), 'ppp0pp'),),
    ('conv', 16, 64, 64, 128, 384, 1, 0, False, False, False, None): (('adm_gemm_x6_amax', (65536, 128, 128, 384, 384, 384, 384), 'pp00pp'),),
    ('conv', 16, 64, 64, 256, 128, 1, 0, True, True, True, None): (('adm_gemm_x6_h3', (65536, 256, 256, 128, 128, 128, 128), 'ppppppp'),),
    ('conv', 16, 64, 64, 256, 128, 3, 1, True, False, False, None): (('adm_conv_fwd_wino2d_x6_up', (0, 16, 128, 128, 256, 256, 128, 128, 128, 128), 'ppp0p0'),),
    ('conv', 16, 64, 64, 256, 256, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (65536, 256, 256, 256, 256, 256, 256), 'ppp0pp'),),
    ('conv', 16, 64, 64, 256, 256, 1, 0, True, True, False, None): (('adm_gemm_x6_amax', (65536, 256, 256, 256, 256, 256, 256), 'pppppp'),),
    ('conv', 16, 64, 64, 256, 256, 3, 0, True, False, False, None): (('adm_conv_fwd_wino2d_x6', (0, 16, 64, 64, 256, 256, 256, 256, 256, 256), 'ppp0p0'),),
    ('conv', 16, 64, 64, 256, 384, 1, 0, False, False, False, None): (('adm_gemm_x6_amax', (65536, 256, 256, 384, 384, 384, 384), 'pp00pp'),),
    ('conv', 16, 64, 64, 384, 256, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (65536, 384, 384, 256, 256, 256, 256), 'ppp0ppp'),),
    ('conv', 16, 64, 64, 384, 256, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 16, 64, 64, 384, 384, 256, 256, 256, 256, 0), 'ppp0p0p'),),
    ('conv', 16, 64, 64, 512, 256, 1, 0, True, True, True, None): (('adm_gemm_x6_h3', (65536, 512, 512, 256, 256, 256, 256), 'ppppppp'),),
    ('conv', 16, 128, 128, 128, 3, 1, 0, True, False, False, None): (('adm_conv_fwd', (16, 128, 128, 128, 128, 32, 32, 32, 32, 1, 0, -1), 'ppp0p'),),
    ('conv', 16, 128, 128, 128, 128, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (262144, 128, 128, 128, 128, 128, 128), 'ppp0pp'),),
    ('conv', 16, 128, 128, 128, 128, 1, 0, True, True, False, None): (('adm_gemm_x6_amax', (262144, 128, 128, 128, 128, 128, 128), 'pppppp'),),
    ('conv', 16, 128, 128, 128, 128, 3, 0, True, False, False, None): (('adm_conv_fwd_wino2d_x6', (0, 16, 128, 128, 128, 128, 128, 128, 128, 128), 'ppp0p0'),),
    ('conv', 16, 128, 128, 128, 128, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 16, 128, 128, 128, 128, 128, 128, 128, 128, 0), 'ppp0p0p'),),
    ('conv', 16, 128, 128, 128, 384, 1, 0, False, False, False, None): (('adm_gemm_x6_amax', (262144, 128, 128, 384, 384, 384, 384), 'pp00pp'),),
    ('conv', 16, 128, 128, 256, 128, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (262144, 256, 256, 128, 128, 128, 128), 'ppp0ppp'),),
    ('conv', 16, 128, 128, 256, 128, 1, 0, True, True, True, None): (('adm_gemm_x6_h3', (262144, 256, 256, 128, 128, 128, 128), 'ppppppp'),),
    ('conv', 16, 128, 128, 256, 128, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 16, 128, 128, 256, 256, 128, 128, 128, 128, 0), 'ppp0p0p'),),
    ('conv', 32, 1, 1, 128, 512, 1, 0, True, False, False, None): (('adm_conv_fwd', (32, 1, 1, 128, 128, 512, 512, 512, 512, 1, 0, -1), 'ppp0p'),),
    ('conv', 32, 1, 1, 512, 256, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (16384, 32, 1, 1, 512, 512, 256, 256, 256, 256, 1, 0), 'ppp0pp'),),
    ('conv', 32, 1, 1, 512, 512, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (32768, 32, 1, 1, 512, 512, 512, 512, 512, 512, 1, 0), 'ppp0pp'),),
    ('conv', 32, 8, 8, 256, 1, 1, 0, True, False, False, None): (('adm_conv_fwd', (32, 8, 8, 256, 256, 32, 32, 32, 32, 1, 0, -1), 'ppp0p'),),
    ('conv', 32, 8, 8, 256, 256, 1, 0, True, True, True, None): (('adm_gemm_x6_h3', (2048, 256, 256, 256, 256, 256, 256), 'ppppppp'),),
    ('conv', 32, 8, 8, 256, 256, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (2097152, 32, 8, 8, 256, 256, 256, 256, 256, 256, 0), 'ppp0ppp'),),
    ('conv', 32, 8, 8, 256, 256, 3, 0, True, True, True, None): (('adm_conv_fwd_wino2d_h3', (2097152, 32, 8, 8, 256, 256, 256, 256, 256, 256, 0), 'ppppppp'),),
    ('conv', 32, 8, 8, 256, 256, 3, 1, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (4194304, 32, 16, 16, 256, 256, 256, 256, 256, 256, 1), 'ppp0ppp'),),
    ('conv', 32, 8, 8, 256, 768, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (2048, 256, 256, 768, 768, 768, 768), 'ppp0ppp'),),
    ('conv', 32, 8, 8, 512, 256, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (2048, 512, 512, 256, 256, 256, 256), 'ppp0ppp'),),
    ('conv', 32, 8, 8, 512, 256, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (3145728, 32, 8, 8, 512, 512, 256, 256, 256, 256, 0), 'ppp0ppp'),),
    ('conv', 32, 16, 16, 256, 256, 1, 0, True, True, True, None): (('adm_gemm_x6_h3', (8192, 256, 256, 256, 256, 256, 256), 'ppppppp'),),
    ('conv', 32, 16, 16, 256, 256, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (4194304, 32, 16, 16, 256, 256, 256, 256, 256, 256, 0), 'ppp0ppp'),),
    ('conv', 32, 16, 16, 256, 256, 3, 0, True, True, True, None): (('adm_conv_fwd_wino2d_h3', (4194304, 32, 16, 16, 256, 256, 256, 256, 256, 256, 0), 'ppppppp'),),
    ('conv', 32, 16, 16, 256, 256, 3, 1, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 256, 256, 256, 256, 256, 256, 1), 'ppp0p0p'),),
    ('conv', 32, 16, 16, 256, 768, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (8192, 256, 256, 768, 768, 768, 768), 'ppp0ppp'),),
    ('conv', 32, 16, 16, 512, 256, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (8192, 512, 512, 256, 256, 256, 256), 'ppp0ppp'),),
    ('conv', 32, 16, 16, 512, 256, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (4194304, 32, 16, 16, 512, 512, 256, 256, 256, 256, 0), 'ppp0ppp'),),
    ('conv', 32, 32, 32, 128, 128, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 128, 128, 128, 128, 128, 128, 0), 'ppp0p0p'),),
    ('conv', 32, 32, 32, 128, 128, 3, 0, True, True, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 128, 128, 128, 128, 128, 128, 0), 'ppppp0p'),),
    ('conv', 32, 32, 32, 128, 256, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (32768, 128, 128, 256, 256, 256, 256), 'ppp0pp'),),
    ('conv', 32, 32, 32, 128, 256, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 128, 128, 256, 256, 256, 256, 0), 'ppp0p0p'),),
    ('conv', 32, 32, 32, 256, 256, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 256, 256, 256, 256, 256, 256, 0), 'ppp0p0p'),),
    ('conv', 32, 32, 32, 256, 256, 3, 0, True, True, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 256, 256, 256, 256, 256, 256, 0), 'ppppp0p'),),
    ('conv', 32, 32, 32, 256, 256, 3, 1, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 256, 256, 256, 256, 256, 256, 1), 'ppp0p0p'),),
    ('conv', 32, 32, 32, 384, 256, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (32768, 384, 384, 256, 256, 256, 256), 'ppp0ppp'),),
    ('conv', 32, 32, 32, 384, 256, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 384, 384, 256, 256, 256, 256, 0), 'ppp0p0p'),),
    ('conv', 32, 32, 32, 512, 256, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (32768, 512, 512, 256, 256, 256, 256), 'ppp0ppp'),),
    ('conv', 32, 32, 32, 512, 256, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 512, 512, 256, 256, 256, 256, 0), 'ppp0p0p'),),
    ('conv', 32, 64, 64, 3, 128, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 32, 32, 128, 128, 128, 128, 0), 'ppp0p0p'),),
    ('conv', 32, 64, 64, 128, 3, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 128, 128, 32, 32, 32, 32, 0), 'ppp0p0p'),),
    ('conv', 32, 64, 64, 128, 128, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 128, 128, 128, 128, 128, 128, 0), 'ppp0p0p'),),
    ('conv', 32, 64, 64, 128, 128, 3, 0, True, True, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 128, 128, 128, 128, 128, 128, 0), 'ppppp0p'),),
    ('conv', 32, 64, 64, 256, 128, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (131072, 256, 256, 128, 128, 128, 128), 'ppp0ppp'),),
    ('conv', 32, 64, 64, 256, 128, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 256, 256, 128, 128, 128, 128, 0), 'ppp0p0p'),),
    ('conv', 32, 64, 64, 256, 256, 3, 0, True, True, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 256, 256, 256, 256, 256, 256, 0), 'ppppp0p'),),
    ('conv', 32, 64, 64, 384, 128, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (131072, 384, 384, 128, 128, 128, 128), 'ppp0ppp'),),
    ('conv', 32, 64, 64, 384, 128, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 384, 384, 128, 128, 128, 128, 0), 'ppp0p0p'),),
    ('conv', 128, 1, 1, 192, 768, 1, 0, True, False, False, None): (('adm_conv_fwd', (128, 1, 1, 192, 192, 768, 768, 768, 768, 1, 0, -1), 'ppp0p'),),
    ('conv', 128, 1, 1, 768, 384, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (147456, 128, 1, 1, 768, 768, 384, 384, 384, 384, 1, 0), 'ppp0pp'),),
    ('conv', 128, 1, 1, 768, 768, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (294912, 128, 1, 1, 768, 768, 768, 768, 768, 768, 1, 0), 'ppp0pp'),),
    ('conv', 128, 4, 4, 384, 1, 1, 0, True, False, False, None): (('adm_conv_fwd', (128, 4, 4, 384, 384, 32, 32, 32, 32, 1, 0, -1), 'ppp0p'),),
    ('conv', 128, 4, 4, 384, 384, 1, 0, True, True, True, None): (('adm_gemm_x6_h3', (2048, 384, 384, 384, 384, 384, 384), 'ppppppp'),),
    ('conv', 128, 4, 4, 384, 384, 3, 0, True, False, False, None): (('adm_conv_fwd_wino2d_x6', (3145728, 128, 4, 4, 384, 384, 384, 384, 384, 384), 'ppp0pp'),),
    ('conv', 128, 4, 4, 384, 384, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (3145728, 128, 4, 4, 384, 384, 384, 384, 384, 384, 0), 'ppp0ppp'),),
    ('conv', 128, 4, 4, 384, 384, 3, 0, True, True, True, None): (('adm_conv_fwd_wino2d_h3', (3145728, 128, 4, 4, 384, 384, 384, 384, 384, 384, 0), 'ppppppp'),),
    ('conv', 128, 4, 4, 384, 384, 3, 1, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 8, 8, 384, 384, 384, 384, 384, 384, 1), 'ppp0p0p'),),
    ('conv', 128, 4, 4, 384, 1152, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (2048, 384, 384, 1152, 1152, 1152, 1152), 'ppp0ppp'),),
    ('conv', 128, 4, 4, 768, 384, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (2048, 768, 768, 384, 384, 384, 384), 'ppp0ppp'),),
    ('conv', 128, 4, 4, 768, 384, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (3932160, 128, 4, 4, 768, 768, 384, 384, 384, 384, 0), 'ppp0ppp'),),
    ('conv', 128, 8, 8, 384, 384, 1, 0, True, True, True, None): (('adm_gemm_x6_h3', (8192, 384, 384, 384, 384, 384, 384), 'ppppppp'),),
    ('conv', 128, 8, 8, 384, 384, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 8, 8, 384, 384, 384, 384, 384, 384, 0), 'ppp0p0p'),),
    ('conv', 128, 8, 8, 384, 384, 3, 0, True, True, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 8, 8, 384, 384, 384, 384, 384, 384, 0), 'ppppp0p'),),
    ('conv', 128, 8, 8, 384, 384, 3, 1, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 384, 384, 384, 384, 384, 384, 1), 'ppp0p0p'),),
    ('conv', 128, 8, 8, 384, 1152, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (8192, 384, 384, 1152, 1152, 1152, 1152), 'ppp0ppp'),),
    ('conv', 128, 8, 8, 768, 384, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (8192, 768, 768, 384, 384, 384, 384), 'ppp0ppp'),),
    ('conv', 128, 8, 8, 768, 384, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 8, 8, 768, 768, 384, 384, 384, 384, 0), 'ppp0p0p'),),
    ('conv', 128, 16, 16, 192, 192, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 192, 192, 192, 192, 192, 192, 0), 'ppp0p0p'),),
    ('conv', 128, 16, 16, 192, 192, 3, 0, True, True, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 192, 192, 192, 192, 192, 192, 0), 'ppppp0p'),),
    ('conv', 128, 16, 16, 192, 384, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (32768, 192, 192, 384, 384, 384, 384), 'ppp0pp'),),
    ('conv', 128, 16, 16, 192, 384, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 192, 192, 384, 384, 384, 384, 0), 'ppp0p0p'),),
    ('conv', 128, 16, 16, 384, 384, 1, 0, True, True, True, None): (('adm_gemm_x6_h3', (32768, 384, 384, 384, 384, 384, 384), 'ppppppp'),),
    ('conv', 128, 16, 16, 384, 384, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 384, 384, 384, 384, 384, 384, 0), 'ppp0p0p'),),
    ('conv', 128, 16, 16, 384, 384, 3, 0, True, True, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 384, 384, 384, 384, 384, 384, 0), 'ppppp0p'),),
    ('conv', 128, 16, 16, 384, 384, 3, 1, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 384, 384, 384, 384, 384, 384, 1), 'ppp0p0p'),),
    ('conv', 128, 16, 16, 384, 1152, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (32768, 384, 384, 1152, 1152, 1152, 1152), 'ppp0ppp'),),
    ('conv', 128, 16, 16, 576, 384, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (32768, 576, 576, 384, 384, 384, 384), 'ppp0ppp'),),
    ('conv', 128, 16, 16, 576, 384, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 576, 576, 384, 384, 384, 384, 0), 'ppp0p0p'),),
    ('conv', 128, 16, 16, 768, 384, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (32768, 768, 768, 384, 384, 384, 384), 'ppp0ppp'),),
    ('conv', 128, 16, 16, 768, 384, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 768, 768, 384, 384, 384, 384, 0), 'ppp0p0p'),),
    ('conv', 128, 32, 32, 3, 192, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 32, 32, 192, 192, 192, 192, 0), 'ppp0p0p'),),
    ('conv', 128, 32, 32, 192, 3, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 192, 192, 32, 32, 32, 32, 0), 'ppp0p0p'),),
    ('conv', 128, 32, 32, 192, 192, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 192, 192, 192, 192, 192, 192, 0), 'ppp0p0p'),),
    ('conv', 128, 32, 32, 192, 192, 3, 0, True, True, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 192, 192, 192, 192, 192, 192, 0), 'ppppp0p'),),
    ('conv', 128, 32, 32, 384, 192, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (131072, 384, 384, 192, 192, 192, 192), 'ppp0ppp'),),
    ('conv', 128, 32, 32, 384, 192, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 384, 384, 192, 192, 192, 192, 0), 'ppp0p0p'),),
    ('conv', 128, 32, 32, 384, 384, 3, 0, True, True, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 384, 384, 384, 384, 384, 384, 0), 'ppppp0p'),),
    ('conv', 128, 32, 32, 576, 192, 1, 0, True, False, True, None): (('adm_gemm_x6_h3', (131072, 576, 576, 192, 192, 192, 192), 'ppp0ppp'),),
    ('conv', 128, 32, 32, 576, 192, 3, 0, True, False, True, None): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 576, 576, 192, 192, 192, 192, 0), 'ppp0p0p'),),
    ('conv', 256, 1, 1, 128, 128, 1, 0, True, False, False, None): (('adm_conv_fwd', (256, 1, 1, 128, 128, 128, 128, 128, 128, 1, 0, -1), 'ppp0p'),),
    ('conv', 256, 1, 1, 256, 256, 1, 0, True, False, False, None): (('adm_conv_fwd', (256, 1, 1, 256, 256, 256, 256, 256, 256, 1, 0, -1), 'ppp0p'),),
    ('conv', 256, 1, 1, 512, 512, 1, 0, True, False, False, None): (('adm_conv_fwd_ws', (262144, 256, 1, 1, 512, 512, 512, 512, 512, 512, 1, 0), 'ppp0pp'),),
    ('conv', 4096, 1, 1, 512, 512, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (4096, 512, 512, 512, 512, 512, 512), 'ppp0pp'),),
    ('conv', 16384, 1, 1, 128, 128, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (16384, 128, 128, 128, 128, 128, 128), 'ppp0pp'),),
    ('conv', 16384, 1, 1, 256, 256, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (16384, 256, 256, 256, 256, 256, 256), 'ppp0pp'),),
    ('conv', 16384, 1, 1, 512, 512, 1, 0, True, False, False, None): (('adm_gemm_x6_amax', (16384, 512, 512, 512, 512, 512, 512), 'ppp0pp'),),
    ('conv-bwd', 16, 1, 1, 128, 512, 1, 0, True, False, False, None, False, False, False, True, True, True, True): (('adm_conv_wgrad_bias', (16, 1, 1, 128, 128, 512, 512, 1, 0, -1), 'pppp'),),
    ('conv-bwd', 16, 1, 1, 128, 512, 1, 0, True, False, False, None, False, True, False, True, True, True, True): (('adm_conv_wgrad_ws', (16, 1, 1, 128, 128, 512, 512, 1, 0, 1, 0), 'pppp'),),
    ('conv-bwd', 16, 1, 1, 512, 256, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd', (16, 1, 1, 256, 256, 512, 512, 512, 512, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_bias', (16, 1, 1, 512, 512, 256, 256, 1, 0, -1), 'pppp')),
    ('conv-bwd', 16, 1, 1, 512, 256, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd', (16, 1, 1, 256, 256, 512, 512, 512, 512, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_ws', (16, 1, 1, 512, 512, 256, 256, 1, 0, 1, 0), 'pppp')),
    ('conv-bwd', 16, 1, 1, 512, 512, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd_ws', (16384, 16, 1, 1, 512, 512, 512, 512, 512, 512, 1, 0), 'pp00pp'), ('adm_conv_wgrad_bias', (16, 1, 1, 512, 512, 512, 512, 1, 0, -1), 'pppp')),
    ('conv-bwd', 16, 1, 1, 512, 512, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd_ws', (16384, 16, 1, 1, 512, 512, 512, 512, 512, 512, 1, 0), 'pp00pp'), ('adm_conv_wgrad_ws', (16, 1, 1, 512, 512, 512, 512, 1, 0, 1, 0), 'pppp')),
    ('conv-bwd', 16, 1, 1, 512, 1024, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd_ws', (32768, 16, 1, 1, 1024, 1024, 512, 512, 512, 512, 1, 0), 'pp00pp'), ('adm_conv_wgrad_bias', (16, 1, 1, 512, 512, 1024, 1024, 1, 0, -1), 'pppp')),
    ('conv-bwd', 16, 1, 1, 512, 1024, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd_ws', (32768, 16, 1, 1, 1024, 1024, 512, 512, 512, 512, 1, 0), 'pp00pp'), ('adm_conv_wgrad_ws', (16, 1, 1, 512, 512, 1024, 1024, 1, 0, 1, 0), 'pppp')),
    ('conv-bwd', 16, 4, 4, 128, 256, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd', (16, 4, 4, 256, 256, 128, 128, 128, 128, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_bias', (16, 4, 4, 128, 128, 256, 256, 1, 0, -1), 'pppp')),
    ('conv-bwd', 16, 4, 4, 128, 256, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd', (16, 4, 4, 256, 256, 128, 128, 128, 128, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_ws', (16, 4, 4, 128, 128, 256, 256, 1, 0, 2, 0), 'pppp')),
    ('conv-bwd', 16, 4, 4, 256, 128, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd', (16, 4, 4, 128, 128, 256, 256, 256, 256, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_bias', (16, 4, 4, 256, 256, 128, 128, 1, 0, -1), 'pppp')),
    ('conv-bwd', 16, 4, 4, 256, 128, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd', (16, 4, 4, 128, 128, 256, 256, 256, 256, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_ws', (16, 4, 4, 256, 256, 128, 128, 1, 0, 2, 0), 'pppp')),
    ('conv-bwd', 16, 4, 4, 256, 512, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd_ws', (131072, 16, 4, 4, 512, 512, 256, 256, 256, 256, 1, 0), 'pp00pp'), ('adm_conv_wgrad_bias', (16, 4, 4, 256, 256, 512, 512, 1, 0, -1), 'pppp')),
    ('conv-bwd', 16, 4, 4, 256, 512, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd_ws', (131072, 16, 4, 4, 512, 512, 256, 256, 256, 256, 1, 0), 'pp00pp'), ('adm_conv_wgrad_ws', (16, 4, 4, 256, 256, 512, 512, 1, 0, 2, 0), 'pppp')),
    ('conv-bwd', 16, 4, 4, 512, 256, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd', (16, 4, 4, 256, 256, 512, 512, 512, 512, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_bias', (16, 4, 4, 512, 512, 256, 256, 1, 0, -1), 'pppp')),
    ('conv-bwd', 16, 4, 4, 512, 256, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd', (16, 4, 4, 256, 256, 512, 512, 512, 512, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_ws', (16, 4, 4, 512, 512, 256, 256, 1, 0, 2, 0), 'pppp')),
    ('conv-bwd', 16, 4, 4, 512, 512, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd_ws', (262144, 16, 4, 4, 512, 512, 512, 512, 512, 512, 1, 0), 'pp00pp'), ('adm_conv_wgrad_bias', (16, 4, 4, 512, 512, 512, 512, 1, 0, -1), 'pppp')),
    ('conv-bwd', 16, 4, 4, 512, 512, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd_ws', (262144, 16, 4, 4, 512, 512, 512, 512, 512, 512, 1, 0), 'pp00pp'), ('adm_conv_wgrad_ws', (16, 4, 4, 512, 512, 512, 512, 1, 0, 2, 0), 'pppp')),
    ('conv-bwd', 16, 4, 4, 512, 1024, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd_ws', (524288, 16, 4, 4, 1024, 1024, 512, 512, 512, 512, 1, 0), 'pp00pp'), ('adm_conv_wgrad_bias', (16, 4, 4, 512, 512, 1024, 1024, 1, 0, -1), 'pppp')),
    ('conv-bwd', 16, 4, 4, 512, 1024, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd_ws', (524288, 16, 4, 4, 1024, 1024, 512, 512, 512, 512, 1, 0), 'pp00pp'), ('adm_conv_wgrad_ws', (16, 4, 4, 512, 512, 1024, 1024, 1, 0, 2, 0), 'pppp')),
    ('conv-bwd', 16, 4, 4, 1024, 512, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd_ws', (524288, 16, 4, 4, 512, 512, 1024, 1024, 1024, 1024, 1, 0), 'pp00pp'), ('adm_conv_wgrad_bias', (16, 4, 4, 1024, 1024, 512, 512, 1, 0, -1), 'pppp')),
    ('conv-bwd', 16, 4, 4, 1024, 512, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd_ws', (524288, 16, 4, 4, 512, 512, 1024, 1024, 1024, 1024, 1, 0), 'pp00pp'), ('adm_conv_wgrad_ws', (16, 4, 4, 1024, 1024, 512, 512, 1, 0, 2, 0), 'pppp')),
    ('conv-bwd', 16, 4, 4, 1024, 512, 1, 0, True, False, True, None, False, False, False, True, True, True, True): (('adm_conv_wgrad_bias', (16, 4, 4, 1024, 1024, 512, 512, 1, 0, -1), 'pppp'),),
    ('conv-bwd', 16, 4, 4, 1024, 512, 1, 0, True, False, True, None, False, True, False, True, True, True, True): (('adm_conv_wgrad_ws', (16, 4, 4, 1024, 1024, 512, 512, 1, 0, 2, 0), 'pppp'),),
    ('conv-bwd', 16, 8, 8, 256, 256, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd', (16, 8, 8, 256, 256, 256, 256, 256, 256, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_bias', (16, 8, 8, 256, 256, 256, 256, 1, 0, -1), 'pppp')),
    ('conv-bwd', 16, 8, 8, 256, 256, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd', (16, 8, 8, 256, 256, 256, 256, 256, 256, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_ws', (16, 8, 8, 256, 256, 256, 256, 1, 0, 8, 0), 'pppp')),
    ('conv-bwd', 16, 8, 8, 256, 512, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd_ws', (524288, 16, 8, 8, 512, 512, 256, 256, 256, 256, 1, 0), 'pp00pp'), ('adm_conv_wgrad_bias', (16, 8, 8, 256, 256, 512, 512, 1, 0, -1), 'pppp')),
    ('conv-bwd', 16, 8, 8, 256, 512, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd_ws', (524288, 16, 8, 8, 512, 512, 256, 256, 256, 256, 1, 0), 'pp00pp'), ('adm_conv_wgrad_ws', (16, 8, 8, 256, 256, 512, 512, 1, 0, 8, 0), 'pppp')),
    ('conv-bwd', 16, 8, 8, 512, 256, 1, 0, True, False, True, None, False, False, False, True, True, True, True): (('adm_conv_wgrad_bias', (16, 8, 8, 512, 512, 256, 256, 1, 0, -1), 'pppp'),),
    ('conv-bwd', 16, 8, 8, 512, 256, 1, 0, True, False, True, None, False, True, False, True, True, True, True): (('adm_conv_wgrad_ws', (16, 8, 8, 512, 512, 256, 256, 1, 0, 8, 0), 'pppp'),),
    ('conv-bwd', 16, 16, 16, 128, 128, 1, 0, True, False, True, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (4096, 128, 128, 128, 128, -1), 'pppp'), ('adm_gemm_x6', (4096, 128, 128, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 128, 128, 1, 0, True, False, True, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (4096, 128, 128, 128, 128, 11), 'pppp'), ('adm_gemm_x6', (4096, 128, 128, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 128, 256, 1, 0, True, False, True, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (4096, 128, 128, 256, 256, -1), 'pppp'), ('adm_gemm_x6', (4096, 256, 256, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 128, 256, 1, 0, True, False, True, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (4096, 128, 128, 256, 256, 11), 'pppp'), ('adm_gemm_x6', (4096, 256, 256, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 128, 512, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (4096, 128, 128, 512, 512, -1), 'pppp'), ('adm_gemm_x6', (4096, 512, 512, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 128, 512, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (4096, 128, 128, 512, 512, 11), 'pppp'), ('adm_gemm_x6', (4096, 512, 512, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 128, 512, 1, 0, True, True, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (4096, 128, 128, 512, 512, -1), 'pppp'), ('adm_gemm_x6', (4096, 512, 512, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 128, 512, 1, 0, True, True, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (4096, 128, 128, 512, 512, 11), 'pppp'), ('adm_gemm_x6', (4096, 512, 512, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 256, 128, 1, 0, True, False, True, None, False, False, False, True, True, True, True): (('adm_gemm_wgrad_x6', (4096, 256, 256, 128, 128, -1), 'pppp'),),
    ('conv-bwd', 16, 16, 16, 256, 128, 1, 0, True, False, True, None, False, True, False, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (4096, 256, 256, 128, 128, 11), 'pppp'),),
    ('conv-bwd', 16, 16, 16, 512, 1, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd', (16, 16, 16, 32, 32, 512, 512, 512, 512, 1, 0, -1), 'pp00p'), ('adm_gemm_wgrad_x6', (4096, 512, 512, 32, 32, -1), 'pppp')),
    ('conv-bwd', 16, 16, 16, 512, 1, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd', (16, 16, 16, 32, 32, 512, 512, 512, 512, 1, 0, -1), 'pp00p'), ('adm_gemm_wgrad_x6_ws', (4096, 512, 512, 32, 32, 11), 'pppp')),
    ('conv-bwd', 16, 16, 16, 512, 384, 1, 0, False, False, False, None, False, False, True, True, False, True, False): (('adm_gemm_wgrad_x6', (4096, 512, 512, 384, 384, -1), 'ppp0'), ('adm_gemm_x6', (4096, 384, 384, 512, 512, 512, 512), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 512, 384, 1, 0, False, False, False, None, False, True, True, True, False, True, False): (('adm_gemm_wgrad_x6_ws', (4096, 512, 512, 384, 384, 5), 'ppp0'), ('adm_gemm_x6', (4096, 384, 384, 512, 512, 512, 512), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 512, 512, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (4096, 512, 512, 512, 512, -1), 'pppp'), ('adm_gemm_x6', (4096, 512, 512, 512, 512, 512, 512), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 512, 512, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (4096, 512, 512, 512, 512, 4), 'pppp'), ('adm_gemm_x6', (4096, 512, 512, 512, 512, 512, 512), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 512, 512, 1, 0, True, True, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (4096, 512, 512, 512, 512, -1), 'pppp'), ('adm_gemm_x6', (4096, 512, 512, 512, 512, 512, 512), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 512, 512, 1, 0, True, True, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (4096, 512, 512, 512, 512, 4), 'pppp'), ('adm_gemm_x6', (4096, 512, 512, 512, 512, 512, 512), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 512, 512, 3, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_x6', (4194304, 16, 16, 16, 512, 512, 512, 512, 512, 512), 'pp00pp'), ('adm_conv_wgrad_x6', (16, 16, 16, 512, 512, 512, 512, -1), 'pppp')),
    ('conv-bwd', 16, 16, 16, 512, 512, 3, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_x6', (4194304, 16, 16, 16, 512, 512, 512, 512, 512, 512), 'pp00pp'), ('adm_conv_wgrad_x6_ws', (16, 16, 16, 512, 512, 512, 512, 1, 0), 'pppp')),
    ('conv-bwd', 16, 16, 16, 512, 512, 3, 0, True, False, False, None, True, False, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (4194304, 16, 16, 16, 512, 512, 512, 512, 512, 512, 0), 'pp00ppp'), ('adm_conv_wgrad_x6', (16, 16, 16, 512, 512, 512, 512, 0), 'pppp')),
    ('conv-bwd', 16, 16, 16, 512, 512, 3, 0, True, False, False, None, True, True, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (4194304, 16, 16, 16, 512, 512, 512, 512, 512, 512, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_ws', (16, 16, 16, 512, 512, 512, 512, 1, 0), 'pppp')),
    ('conv-bwd', 16, 16, 16, 512, 512, 3, 0, True, False, True, None, True, False, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (4194304, 16, 16, 16, 512, 512, 512, 512, 512, 512, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (16, 16, 16, 512, 512, 512, 512, 0, 0, 0), 'pppppp')),
    ('conv-bwd', 16, 16, 16, 512, 512, 3, 0, True, False, True, None, True, True, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (4194304, 16, 16, 16, 512, 512, 512, 512, 512, 512, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (16, 16, 16, 512, 512, 512, 512, 1, 0, 1), 'pppppp')),
    ('conv-bwd', 16, 16, 16, 512, 512, 3, 1, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_x6', (0, 16, 32, 32, 512, 512, 512, 512, 512, 512), 'pp00p0'), ('adm_conv_wgrad_x6_up', (16, 32, 32, 512, 512, 512, 512, -1), 'pppp')),
    ('conv-bwd', 16, 16, 16, 512, 512, 3, 1, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_x6', (0, 16, 32, 32, 512, 512, 512, 512, 512, 512), 'pp00p0'), ('adm_conv_wgrad_x6_ws', (16, 32, 32, 512, 512, 512, 512, 1, 1), 'pppp')),
    ('conv-bwd', 16, 16, 16, 1024, 512, 1, 0, True, False, True, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (4096, 1024, 1024, 512, 512, -1), 'pppp'), ('adm_gemm_x6', (4096, 512, 512, 1024, 1024, 1024, 1024), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 1024, 512, 1, 0, True, False, True, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (4096, 1024, 1024, 512, 512, 2), 'pppp'), ('adm_gemm_x6', (4096, 512, 512, 1024, 1024, 1024, 1024), 'pp00p')),
    ('conv-bwd', 16, 16, 16, 1024, 512, 1, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (4096, 1024, 1024, 512, 512, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (4096, 512, 512, 1024, 1024, 1024, 1024), 'pp00ppp')),
    ('conv-bwd', 16, 16, 16, 1024, 512, 1, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (4096, 1024, 1024, 512, 512, 2, 1), 'pppppp'), ('adm_gemm_x6_h3', (4096, 512, 512, 1024, 1024, 1024, 1024), 'pp00ppp')),
    ('conv-bwd', 16, 16, 16, 1024, 512, 3, 0, True, False, True, None, True, False, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 16, 16, 512, 512, 1024, 1024, 1024, 1024, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (16, 16, 16, 1024, 1024, 512, 512, 0, 0, 0), 'pppppp')),
    ('conv-bwd', 16, 16, 16, 1024, 512, 3, 0, True, False, True, None, True, True, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 16, 16, 512, 512, 1024, 1024, 1024, 1024, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (16, 16, 16, 1024, 1024, 512, 512, 1, 0, 1), 'pppppp')),
    ('conv-bwd', 16, 32, 32, 128, 128, 1, 0, True, False, True, None, False, False, False, True, True, True, True): (('adm_gemm_wgrad_x6', (16384, 128, 128, 128, 128, -1), 'pppp'),),
    ('conv-bwd', 16, 32, 32, 128, 128, 1, 0, True, False, True, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (16384, 128, 128, 128, 128, -1), 'pppp'), ('adm_gemm_x6', (16384, 128, 128, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 128, 128, 1, 0, True, False, True, None, False, True, False, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (16384, 128, 128, 128, 128, 43), 'pppp'),),
    ('conv-bwd', 16, 32, 32, 128, 128, 1, 0, True, False, True, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (16384, 128, 128, 128, 128, 43), 'pppp'), ('adm_gemm_x6', (16384, 128, 128, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 128, 256, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (16384, 128, 128, 256, 256, -1), 'pppp'), ('adm_gemm_x6', (16384, 256, 256, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 128, 256, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (16384, 128, 128, 256, 256, 32), 'pppp'), ('adm_gemm_x6', (16384, 256, 256, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 128, 512, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (16384, 128, 128, 512, 512, -1), 'pppp'), ('adm_gemm_x6', (16384, 512, 512, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 128, 512, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (16384, 128, 128, 512, 512, 16), 'pppp'), ('adm_gemm_x6', (16384, 512, 512, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 256, 256, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (16384, 256, 256, 256, 256, -1), 'pppp'), ('adm_gemm_x6', (16384, 256, 256, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 256, 256, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (16384, 256, 256, 256, 256, 16), 'pppp'), ('adm_gemm_x6', (16384, 256, 256, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 256, 256, 1, 0, True, True, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (16384, 256, 256, 256, 256, -1), 'pppp'), ('adm_gemm_x6', (16384, 256, 256, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 256, 256, 1, 0, True, True, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (16384, 256, 256, 256, 256, 16), 'pppp'), ('adm_gemm_x6', (16384, 256, 256, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 256, 256, 3, 0, True, False, False, None, True, False, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 32, 32, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6', (16, 32, 32, 256, 256, 256, 256, 0), 'pppp')),
    ('conv-bwd', 16, 32, 32, 256, 256, 3, 0, True, False, False, None, True, True, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 32, 32, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_ws', (16, 32, 32, 256, 256, 256, 256, 4, 0), 'pppp')),
    ('conv-bwd', 16, 32, 32, 256, 256, 3, 0, True, False, True, None, True, False, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 32, 32, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (16, 32, 32, 256, 256, 256, 256, 0, 0, 0), 'pppppp')),
    ('conv-bwd', 16, 32, 32, 256, 256, 3, 0, True, False, True, None, True, True, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 32, 32, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (16, 32, 32, 256, 256, 256, 256, 4, 0, 1), 'pppppp')),
    ('conv-bwd', 16, 32, 32, 256, 384, 1, 0, False, False, False, None, False, False, True, True, False, True, False): (('adm_gemm_wgrad_x6', (16384, 256, 256, 384, 384, -1), 'ppp0'), ('adm_gemm_x6', (16384, 384, 384, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 256, 384, 1, 0, False, False, False, None, False, True, True, True, False, True, False): (('adm_gemm_wgrad_x6_ws', (16384, 256, 256, 384, 384, 32), 'ppp0'), ('adm_gemm_x6', (16384, 384, 384, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 512, 256, 1, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (16384, 512, 512, 256, 256, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (16384, 256, 256, 512, 512, 512, 512), 'pp00ppp')),
    ('conv-bwd', 16, 32, 32, 512, 256, 1, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (16384, 512, 512, 256, 256, 8, 1), 'pppppp'), ('adm_gemm_x6_h3', (16384, 256, 256, 512, 512, 512, 512), 'pp00ppp')),
    ('conv-bwd', 16, 32, 32, 512, 256, 3, 1, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_x6', (0, 16, 64, 64, 256, 256, 512, 512, 512, 512), 'pp00p0'), ('adm_conv_wgrad_x6_up', (16, 64, 64, 512, 512, 256, 256, -1), 'pppp')),
    ('conv-bwd', 16, 32, 32, 512, 256, 3, 1, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_x6', (0, 16, 64, 64, 256, 256, 512, 512, 512, 512), 'pp00p0'), ('adm_conv_wgrad_x6_ws', (16, 64, 64, 512, 512, 256, 256, 2, 1), 'pppp')),
    ('conv-bwd', 16, 32, 32, 512, 384, 1, 0, False, False, False, None, False, False, True, True, False, True, False): (('adm_gemm_wgrad_x6', (16384, 512, 512, 384, 384, -1), 'ppp0'), ('adm_gemm_x6', (16384, 384, 384, 512, 512, 512, 512), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 512, 384, 1, 0, False, False, False, None, False, True, True, True, False, True, False): (('adm_gemm_wgrad_x6_ws', (16384, 512, 512, 384, 384, 16), 'ppp0'), ('adm_gemm_x6', (16384, 384, 384, 512, 512, 512, 512), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 512, 512, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (16384, 512, 512, 512, 512, -1), 'pppp'), ('adm_gemm_x6', (16384, 512, 512, 512, 512, 512, 512), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 512, 512, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (16384, 512, 512, 512, 512, 4), 'pppp'), ('adm_gemm_x6', (16384, 512, 512, 512, 512, 512, 512), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 512, 512, 1, 0, True, True, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (16384, 512, 512, 512, 512, -1), 'pppp'), ('adm_gemm_x6', (16384, 512, 512, 512, 512, 512, 512), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 512, 512, 1, 0, True, True, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (16384, 512, 512, 512, 512, 4), 'pppp'), ('adm_gemm_x6', (16384, 512, 512, 512, 512, 512, 512), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 512, 512, 3, 0, True, False, False, None, True, False, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 32, 32, 512, 512, 512, 512, 512, 512, 0), 'pp00p0p'), ('adm_conv_wgrad_x6', (16, 32, 32, 512, 512, 512, 512, 0), 'pppp')),
    ('conv-bwd', 16, 32, 32, 512, 512, 3, 0, True, False, False, None, True, True, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 32, 32, 512, 512, 512, 512, 512, 512, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_ws', (16, 32, 32, 512, 512, 512, 512, 1, 0), 'pppp')),
    ('conv-bwd', 16, 32, 32, 768, 512, 1, 0, True, False, True, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (16384, 768, 768, 512, 512, -1), 'pppp'), ('adm_gemm_x6', (16384, 512, 512, 768, 768, 768, 768), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 768, 512, 1, 0, True, False, True, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (16384, 768, 768, 512, 512, 8), 'pppp'), ('adm_gemm_x6', (16384, 512, 512, 768, 768, 768, 768), 'pp00p')),
    ('conv-bwd', 16, 32, 32, 768, 512, 3, 0, True, False, True, None, True, False, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 32, 32, 512, 512, 768, 768, 768, 768, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (16, 32, 32, 768, 768, 512, 512, 0, 0, 0), 'pppppp')),
    ('conv-bwd', 16, 32, 32, 768, 512, 3, 0, True, False, True, None, True, True, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 32, 32, 512, 512, 768, 768, 768, 768, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (16, 32, 32, 768, 768, 512, 512, 2, 0, 1), 'pppppp')),
    ('conv-bwd', 16, 32, 32, 1024, 512, 1, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (16384, 1024, 1024, 512, 512, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (16384, 512, 512, 1024, 1024, 1024, 1024), 'pp00ppp')),
    ('conv-bwd', 16, 32, 32, 1024, 512, 1, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (16384, 1024, 1024, 512, 512, 2, 1), 'pppppp'), ('adm_gemm_x6_h3', (16384, 512, 512, 1024, 1024, 1024, 1024), 'pp00ppp')),
    ('conv-bwd', 16, 64, 64, 128, 128, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (65536, 128, 128, 128, 128, -1), 'pppp'), ('adm_gemm_x6', (65536, 128, 128, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 128, 128, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (65536, 128, 128, 128, 128, 64), 'pppp'), ('adm_gemm_x6', (65536, 128, 128, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 128, 128, 1, 0, True, True, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (65536, 128, 128, 128, 128, -1), 'pppp'), ('adm_gemm_x6', (65536, 128, 128, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 128, 128, 1, 0, True, True, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (65536, 128, 128, 128, 128, 64), 'pppp'), ('adm_gemm_x6', (65536, 128, 128, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 128, 128, 3, 0, True, False, False, None, True, False, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 64, 64, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6', (16, 64, 64, 128, 128, 128, 128, 0), 'pppp')),
    ('conv-bwd', 16, 64, 64, 128, 128, 3, 0, True, False, False, None, True, True, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 64, 64, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_ws', (16, 64, 64, 128, 128, 128, 128, 16, 0), 'pppp')),
    ('conv-bwd', 16, 64, 64, 128, 128, 3, 0, True, False, True, None, True, False, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 64, 64, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (16, 64, 64, 128, 128, 128, 128, 0, 0, 0), 'pppppp')),
    ('conv-bwd', 16, 64, 64, 128, 128, 3, 0, True, False, True, None, True, True, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 64, 64, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (16, 64, 64, 128, 128, 128, 128, 16, 0, 1), 'pppppp')),
    ('conv-bwd', 16, 64, 64, 128, 256, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (65536, 128, 128, 256, 256, -1), 'pppp'), ('adm_gemm_x6', (65536, 256, 256, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 128, 256, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (65536, 128, 128, 256, 256, 32), 'pppp'), ('adm_gemm_x6', (65536, 256, 256, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 128, 384, 1, 0, False, False, False, None, False, False, True, True, False, True, False): (('adm_gemm_wgrad_x6', (65536, 128, 128, 384, 384, -1), 'ppp0'), ('adm_gemm_x6', (65536, 384, 384, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 128, 384, 1, 0, False, False, False, None, False, True, True, True, False, True, False): (('adm_gemm_wgrad_x6_ws', (65536, 128, 128, 384, 384, 21), 'ppp0'), ('adm_gemm_x6', (65536, 384, 384, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 256, 128, 1, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (65536, 256, 256, 128, 128, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (65536, 128, 128, 256, 256, 256, 256), 'pp00ppp')),
    ('conv-bwd', 16, 64, 64, 256, 128, 1, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (65536, 256, 256, 128, 128, 32, 1), 'pppppp'), ('adm_gemm_x6_h3', (65536, 128, 128, 256, 256, 256, 256), 'pp00ppp')),
    ('conv-bwd', 16, 64, 64, 256, 128, 3, 1, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_x6', (0, 16, 128, 128, 128, 128, 256, 256, 256, 256), 'pp00p0'), ('adm_conv_wgrad_x6_up', (16, 128, 128, 256, 256, 128, 128, -1), 'pppp')),
    ('conv-bwd', 16, 64, 64, 256, 128, 3, 1, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_x6', (0, 16, 128, 128, 128, 128, 256, 256, 256, 256), 'pp00p0'), ('adm_conv_wgrad_x6_ws', (16, 128, 128, 256, 256, 128, 128, 8, 1), 'pppp')),
    ('conv-bwd', 16, 64, 64, 256, 256, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (65536, 256, 256, 256, 256, -1), 'pppp'), ('adm_gemm_x6', (65536, 256, 256, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 256, 256, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (65536, 256, 256, 256, 256, 16), 'pppp'), ('adm_gemm_x6', (65536, 256, 256, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 256, 256, 1, 0, True, True, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (65536, 256, 256, 256, 256, -1), 'pppp'), ('adm_gemm_x6', (65536, 256, 256, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 256, 256, 1, 0, True, True, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (65536, 256, 256, 256, 256, 16), 'pppp'), ('adm_gemm_x6', (65536, 256, 256, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 256, 256, 3, 0, True, False, False, None, True, False, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 64, 64, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6', (16, 64, 64, 256, 256, 256, 256, 0), 'pppp')),
    ('conv-bwd', 16, 64, 64, 256, 256, 3, 0, True, False, False, None, True, True, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 64, 64, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_ws', (16, 64, 64, 256, 256, 256, 256, 4, 0), 'pppp')),
    ('conv-bwd', 16, 64, 64, 256, 384, 1, 0, False, False, False, None, False, False, True, True, False, True, False): (('adm_gemm_wgrad_x6', (65536, 256, 256, 384, 384, -1), 'ppp0'), ('adm_gemm_x6', (65536, 384, 384, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 256, 384, 1, 0, False, False, False, None, False, True, True, True, False, True, False): (('adm_gemm_wgrad_x6_ws', (65536, 256, 256, 384, 384, 32), 'ppp0'), ('adm_gemm_x6', (65536, 384, 384, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 384, 256, 1, 0, True, False, True, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (65536, 384, 384, 256, 256, -1), 'pppp'), ('adm_gemm_x6', (65536, 256, 256, 384, 384, 384, 384), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 384, 256, 1, 0, True, False, True, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (65536, 384, 384, 256, 256, 32), 'pppp'), ('adm_gemm_x6', (65536, 256, 256, 384, 384, 384, 384), 'pp00p')),
    ('conv-bwd', 16, 64, 64, 384, 256, 3, 0, True, False, True, None, True, False, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 64, 64, 256, 256, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (16, 64, 64, 384, 384, 256, 256, 0, 0, 0), 'pppppp')),
    ('conv-bwd', 16, 64, 64, 384, 256, 3, 0, True, False, True, None, True, True, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 64, 64, 256, 256, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (16, 64, 64, 384, 384, 256, 256, 8, 0, 1), 'pppppp')),
    ('conv-bwd', 16, 64, 64, 512, 256, 1, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (65536, 512, 512, 256, 256, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (65536, 256, 256, 512, 512, 512, 512), 'pp00ppp')),
    ('conv-bwd', 16, 64, 64, 512, 256, 1, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (65536, 512, 512, 256, 256, 8, 1), 'pppppp'), ('adm_gemm_x6_h3', (65536, 256, 256, 512, 512, 512, 512), 'pp00ppp')),
    ('conv-bwd', 16, 128, 128, 128, 3, 1, 0, True, False, False, None, True, False, True, True, True, True, True): (('adm_conv_fwd', (16, 128, 128, 32, 32, 128, 128, 128, 128, 1, 0, -1), 'pp00p'), ('adm_gemm_wgrad_x6', (262144, 128, 128, 32, 32, -1), 'pppp')),
    ('conv-bwd', 16, 128, 128, 128, 3, 1, 0, True, False, False, None, True, True, True, True, True, True, True): (('adm_conv_fwd', (16, 128, 128, 32, 32, 128, 128, 128, 128, 1, 0, -1), 'pp00p'), ('adm_gemm_wgrad_x6_ws', (262144, 128, 128, 32, 32, 128), 'pppp')),
    ('conv-bwd', 16, 128, 128, 128, 128, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (262144, 128, 128, 128, 128, -1), 'pppp'), ('adm_gemm_x6', (262144, 128, 128, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 128, 128, 128, 128, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (262144, 128, 128, 128, 128, 64), 'pppp'), ('adm_gemm_x6', (262144, 128, 128, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 128, 128, 128, 128, 1, 0, True, True, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (262144, 128, 128, 128, 128, -1), 'pppp'), ('adm_gemm_x6', (262144, 128, 128, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 128, 128, 128, 128, 1, 0, True, True, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (262144, 128, 128, 128, 128, 64), 'pppp'), ('adm_gemm_x6', (262144, 128, 128, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 128, 128, 128, 128, 3, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_x6', (0, 16, 128, 128, 128, 128, 128, 128, 128, 128), 'pp00p0'), ('adm_conv_wgrad_x6', (16, 128, 128, 128, 128, 128, 128, -1), 'pppp')),
    ('conv-bwd', 16, 128, 128, 128, 128, 3, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_x6', (0, 16, 128, 128, 128, 128, 128, 128, 128, 128), 'pp00p0'), ('adm_conv_wgrad_x6_ws', (16, 128, 128, 128, 128, 128, 128, 16, 0), 'pppp')),
    ('conv-bwd', 16, 128, 128, 128, 128, 3, 0, True, False, False, None, True, False, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 128, 128, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6', (16, 128, 128, 128, 128, 128, 128, 0), 'pppp')),
    ('conv-bwd', 16, 128, 128, 128, 128, 3, 0, True, False, False, None, True, True, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 128, 128, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_ws', (16, 128, 128, 128, 128, 128, 128, 16, 0), 'pppp')),
    ('conv-bwd', 16, 128, 128, 128, 128, 3, 0, True, False, True, None, True, False, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 128, 128, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (16, 128, 128, 128, 128, 128, 128, 0, 0, 0), 'pppppp')),
    ('conv-bwd', 16, 128, 128, 128, 128, 3, 0, True, False, True, None, True, True, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 128, 128, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (16, 128, 128, 128, 128, 128, 128, 16, 0, 1), 'pppppp')),
    ('conv-bwd', 16, 128, 128, 128, 384, 1, 0, False, False, False, None, False, False, True, True, False, True, False): (('adm_gemm_wgrad_x6', (262144, 128, 128, 384, 384, -1), 'ppp0'), ('adm_gemm_x6', (262144, 384, 384, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 128, 128, 128, 384, 1, 0, False, False, False, None, False, True, True, True, False, True, False): (('adm_gemm_wgrad_x6_ws', (262144, 128, 128, 384, 384, 21), 'ppp0'), ('adm_gemm_x6', (262144, 384, 384, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16, 128, 128, 256, 128, 1, 0, True, False, True, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (262144, 256, 256, 128, 128, -1), 'pppp'), ('adm_gemm_x6', (262144, 128, 128, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16, 128, 128, 256, 128, 1, 0, True, False, True, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (262144, 256, 256, 128, 128, 32), 'pppp'), ('adm_gemm_x6', (262144, 128, 128, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16, 128, 128, 256, 128, 1, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (262144, 256, 256, 128, 128, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (262144, 128, 128, 256, 256, 256, 256), 'pp00ppp')),
    ('conv-bwd', 16, 128, 128, 256, 128, 1, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (262144, 256, 256, 128, 128, 32, 1), 'pppppp'), ('adm_gemm_x6_h3', (262144, 128, 128, 256, 256, 256, 256), 'pp00ppp')),
    ('conv-bwd', 16, 128, 128, 256, 128, 3, 0, True, False, True, None, True, False, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 128, 128, 128, 128, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (16, 128, 128, 256, 256, 128, 128, 0, 0, 0), 'pppppp')),
    ('conv-bwd', 16, 128, 128, 256, 128, 3, 0, True, False, True, None, True, True, True, True, True, False, True): (('adm_conv_fwd_wino2d_h3', (0, 16, 128, 128, 128, 128, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (16, 128, 128, 256, 256, 128, 128, 8, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 1, 1, 128, 512, 1, 0, True, False, False, None, False, False, False, True, True, True, True): (('adm_conv_wgrad_bias', (32, 1, 1, 128, 128, 512, 512, 1, 0, -1), 'pppp'),),
    ('conv-bwd', 32, 1, 1, 128, 512, 1, 0, True, False, False, None, False, True, False, True, True, True, True): (('adm_conv_wgrad_ws', (32, 1, 1, 128, 128, 512, 512, 1, 0, 1, 0), 'pppp'),),
    ('conv-bwd', 32, 1, 1, 512, 256, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd', (32, 1, 1, 256, 256, 512, 512, 512, 512, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_ws', (32, 1, 1, 512, 512, 256, 256, 1, 0, 1, 0), 'pppp')),
    ('conv-bwd', 32, 1, 1, 512, 512, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd_ws', (32768, 32, 1, 1, 512, 512, 512, 512, 512, 512, 1, 0), 'pp00pp'), ('adm_conv_wgrad_bias', (32, 1, 1, 512, 512, 512, 512, 1, 0, -1), 'pppp')),
    ('conv-bwd', 32, 1, 1, 512, 512, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd_ws', (32768, 32, 1, 1, 512, 512, 512, 512, 512, 512, 1, 0), 'pp00pp'), ('adm_conv_wgrad_ws', (32, 1, 1, 512, 512, 512, 512, 1, 0, 1, 0), 'pppp')),
    ('conv-bwd', 32, 8, 8, 256, 1, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd', (32, 8, 8, 32, 32, 256, 256, 256, 256, 1, 0, -1), 'pp00p'), ('adm_gemm_wgrad_x6', (2048, 256, 256, 32, 32, -1), 'pppp')),
    ('conv-bwd', 32, 8, 8, 256, 1, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd', (32, 8, 8, 32, 32, 256, 256, 256, 256, 1, 0, -1), 'pp00p'), ('adm_gemm_wgrad_x6_ws', (2048, 256, 256, 32, 32, 6), 'pppp')),
    ('conv-bwd', 32, 8, 8, 256, 256, 1, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (2048, 256, 256, 256, 256, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (2048, 256, 256, 256, 256, 256, 256), 'pp00ppp')),
    ('conv-bwd', 32, 8, 8, 256, 256, 1, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (2048, 256, 256, 256, 256, 6, 1), 'pppppp'), ('adm_gemm_x6_h3', (2048, 256, 256, 256, 256, 256, 256), 'pp00ppp')),
    ('conv-bwd', 32, 8, 8, 256, 256, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (2097152, 32, 8, 8, 256, 256, 256, 256, 256, 256, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (32, 8, 8, 256, 256, 256, 256, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 8, 8, 256, 256, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (2097152, 32, 8, 8, 256, 256, 256, 256, 256, 256, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (32, 8, 8, 256, 256, 256, 256, 4, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 8, 8, 256, 256, 3, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (2097152, 32, 8, 8, 256, 256, 256, 256, 256, 256, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (32, 8, 8, 256, 256, 256, 256, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 8, 8, 256, 256, 3, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (2097152, 32, 8, 8, 256, 256, 256, 256, 256, 256, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (32, 8, 8, 256, 256, 256, 256, 4, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 8, 8, 256, 256, 3, 1, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (4194304, 32, 16, 16, 256, 256, 256, 256, 256, 256, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (32, 16, 16, 256, 256, 256, 256, -1, 1, 0), 'pppppp')),
    ('conv-bwd', 32, 8, 8, 256, 256, 3, 1, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (4194304, 32, 16, 16, 256, 256, 256, 256, 256, 256, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (32, 16, 16, 256, 256, 256, 256, 4, 1, 1), 'pppppp')),
    ('conv-bwd', 32, 8, 8, 256, 768, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (2048, 256, 256, 768, 768, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (2048, 768, 768, 256, 256, 256, 256), 'pp00ppp')),
    ('conv-bwd', 32, 8, 8, 256, 768, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (2048, 256, 256, 768, 768, 5, 1), 'pppppp'), ('adm_gemm_x6_h3', (2048, 768, 768, 256, 256, 256, 256), 'pp00ppp')),
    ('conv-bwd', 32, 8, 8, 512, 256, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (2048, 512, 512, 256, 256, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (2048, 256, 256, 512, 512, 512, 512), 'pp00ppp')),
    ('conv-bwd', 32, 8, 8, 512, 256, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (2048, 512, 512, 256, 256, 6, 1), 'pppppp'), ('adm_gemm_x6_h3', (2048, 256, 256, 512, 512, 512, 512), 'pp00ppp')),
    ('conv-bwd', 32, 8, 8, 512, 256, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (4194304, 32, 8, 8, 256, 256, 512, 512, 512, 512, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (32, 8, 8, 512, 512, 256, 256, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 8, 8, 512, 256, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (4194304, 32, 8, 8, 256, 256, 512, 512, 512, 512, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (32, 8, 8, 512, 512, 256, 256, 2, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 16, 16, 256, 256, 1, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (8192, 256, 256, 256, 256, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (8192, 256, 256, 256, 256, 256, 256), 'pp00ppp')),
    ('conv-bwd', 32, 16, 16, 256, 256, 1, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (8192, 256, 256, 256, 256, 16, 1), 'pppppp'), ('adm_gemm_x6_h3', (8192, 256, 256, 256, 256, 256, 256), 'pp00ppp')),
    ('conv-bwd', 32, 16, 16, 256, 256, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (4194304, 32, 16, 16, 256, 256, 256, 256, 256, 256, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (32, 16, 16, 256, 256, 256, 256, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 16, 16, 256, 256, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (4194304, 32, 16, 16, 256, 256, 256, 256, 256, 256, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (32, 16, 16, 256, 256, 256, 256, 4, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 16, 16, 256, 256, 3, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (4194304, 32, 16, 16, 256, 256, 256, 256, 256, 256, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (32, 16, 16, 256, 256, 256, 256, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 16, 16, 256, 256, 3, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (4194304, 32, 16, 16, 256, 256, 256, 256, 256, 256, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (32, 16, 16, 256, 256, 256, 256, 4, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 16, 16, 256, 256, 3, 1, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 256, 256, 256, 256, -1, 1, 0), 'pppppp')),
    ('conv-bwd', 32, 16, 16, 256, 256, 3, 1, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 256, 256, 256, 256, 4, 1, 1), 'pppppp')),
    ('conv-bwd', 32, 16, 16, 256, 768, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (8192, 256, 256, 768, 768, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (8192, 768, 768, 256, 256, 256, 256), 'pp00ppp')),
    ('conv-bwd', 32, 16, 16, 256, 768, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (8192, 256, 256, 768, 768, 16, 1), 'pppppp'), ('adm_gemm_x6_h3', (8192, 768, 768, 256, 256, 256, 256), 'pp00ppp')),
    ('conv-bwd', 32, 16, 16, 512, 256, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (8192, 512, 512, 256, 256, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (8192, 256, 256, 512, 512, 512, 512), 'pp00ppp')),
    ('conv-bwd', 32, 16, 16, 512, 256, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (8192, 512, 512, 256, 256, 8, 1), 'pppppp'), ('adm_gemm_x6_h3', (8192, 256, 256, 512, 512, 512, 512), 'pp00ppp')),
    ('conv-bwd', 32, 16, 16, 512, 256, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 16, 16, 256, 256, 512, 512, 512, 512, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 16, 16, 512, 512, 256, 256, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 16, 16, 512, 256, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 16, 16, 256, 256, 512, 512, 512, 512, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 16, 16, 512, 512, 256, 256, 2, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 128, 128, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 128, 128, 128, 128, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 128, 128, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 128, 128, 128, 128, 16, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 128, 128, 3, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 128, 128, 128, 128, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 128, 128, 3, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 128, 128, 128, 128, 16, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 128, 256, 1, 0, True, False, False, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (32768, 128, 128, 256, 256, -1), 'pppp'), ('adm_gemm_x6_h3', (32768, 256, 256, 128, 128, 128, 128), 'pp00ppp')),
    ('conv-bwd', 32, 32, 32, 128, 256, 1, 0, True, False, False, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (32768, 128, 128, 256, 256, 32), 'pppp'), ('adm_gemm_x6_h3', (32768, 256, 256, 128, 128, 128, 128), 'pp00ppp')),
    ('conv-bwd', 32, 32, 32, 128, 256, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 256, 256, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 128, 128, 256, 256, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 128, 256, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 256, 256, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 128, 128, 256, 256, 8, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 256, 256, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 256, 256, 256, 256, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 256, 256, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 256, 256, 256, 256, 4, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 256, 256, 3, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 256, 256, 256, 256, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 256, 256, 3, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 256, 256, 256, 256, 4, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 256, 256, 3, 1, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 64, 64, 256, 256, 256, 256, -1, 1, 0), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 256, 256, 3, 1, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 64, 64, 256, 256, 256, 256, 4, 1, 1), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 384, 256, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (32768, 384, 384, 256, 256, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (32768, 256, 256, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 32, 32, 32, 384, 256, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (32768, 384, 384, 256, 256, 32, 1), 'pppppp'), ('adm_gemm_x6_h3', (32768, 256, 256, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 32, 32, 32, 384, 256, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 256, 256, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 384, 384, 256, 256, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 384, 256, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 256, 256, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 384, 384, 256, 256, 8, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 512, 256, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (32768, 512, 512, 256, 256, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (32768, 256, 256, 512, 512, 512, 512), 'pp00ppp')),
    ('conv-bwd', 32, 32, 32, 512, 256, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (32768, 512, 512, 256, 256, 8, 1), 'pppppp'), ('adm_gemm_x6_h3', (32768, 256, 256, 512, 512, 512, 512), 'pp00ppp')),
    ('conv-bwd', 32, 32, 32, 512, 256, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 256, 256, 512, 512, 512, 512, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 512, 512, 256, 256, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 32, 32, 512, 256, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 32, 32, 256, 256, 512, 512, 512, 512, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 32, 32, 512, 512, 256, 256, 2, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 64, 64, 3, 128, 3, 0, True, False, True, None, True, False, False, True, True, True, True): (('adm_conv_wgrad_x6_h3', (32, 64, 64, 32, 32, 128, 128, -1, 0, 0), 'pppppp'),),
    ('conv-bwd', 32, 64, 64, 3, 128, 3, 0, True, False, True, None, True, True, False, True, True, True, True): (('adm_conv_wgrad_x6_h3', (32, 64, 64, 32, 32, 128, 128, 32, 0, 1), 'pppppp'),),
    ('conv-bwd', 32, 64, 64, 128, 3, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 32, 32, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 64, 64, 128, 128, 32, 32, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 64, 64, 128, 3, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 32, 32, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 64, 64, 128, 128, 32, 32, 32, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 64, 64, 128, 128, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 64, 64, 128, 128, 128, 128, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 64, 64, 128, 128, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 64, 64, 128, 128, 128, 128, 16, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 64, 64, 128, 128, 3, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 64, 64, 128, 128, 128, 128, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 64, 64, 128, 128, 3, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 128, 128, 128, 128, 128, 128, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 64, 64, 128, 128, 128, 128, 16, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 64, 64, 256, 128, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (131072, 256, 256, 128, 128, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (131072, 128, 128, 256, 256, 256, 256), 'pp00ppp')),
    ('conv-bwd', 32, 64, 64, 256, 128, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (131072, 256, 256, 128, 128, 32, 1), 'pppppp'), ('adm_gemm_x6_h3', (131072, 128, 128, 256, 256, 256, 256), 'pp00ppp')),
    ('conv-bwd', 32, 64, 64, 256, 128, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 128, 128, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 64, 64, 256, 256, 128, 128, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 64, 64, 256, 128, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 128, 128, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 64, 64, 256, 256, 128, 128, 8, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 64, 64, 256, 256, 3, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 64, 64, 256, 256, 256, 256, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 64, 64, 256, 256, 3, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 256, 256, 256, 256, 256, 256, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 64, 64, 256, 256, 256, 256, 4, 0, 1), 'pppppp')),
    ('conv-bwd', 32, 64, 64, 384, 128, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (131072, 384, 384, 128, 128, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (131072, 128, 128, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 32, 64, 64, 384, 128, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (131072, 384, 384, 128, 128, 21, 1), 'pppppp'), ('adm_gemm_x6_h3', (131072, 128, 128, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 32, 64, 64, 384, 128, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 128, 128, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 64, 64, 384, 384, 128, 128, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 32, 64, 64, 384, 128, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 32, 64, 64, 128, 128, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (32, 64, 64, 384, 384, 128, 128, 16, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 1, 1, 192, 768, 1, 0, True, False, False, None, False, False, False, True, True, True, True): (('adm_conv_wgrad_bias', (128, 1, 1, 192, 192, 768, 768, 1, 0, -1), 'pppp'),),
    ('conv-bwd', 128, 1, 1, 192, 768, 1, 0, True, False, False, None, False, True, False, True, True, True, True): (('adm_conv_wgrad_ws', (128, 1, 1, 192, 192, 768, 768, 1, 0, 1, 0), 'pppp'),),
    ('conv-bwd', 128, 1, 1, 768, 384, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd', (128, 1, 1, 384, 384, 768, 768, 768, 768, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_ws', (128, 1, 1, 768, 768, 384, 384, 1, 0, 1, 0), 'pppp')),
    ('conv-bwd', 128, 1, 1, 768, 768, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd_ws', (294912, 128, 1, 1, 768, 768, 768, 768, 768, 768, 1, 0), 'pp00pp'), ('adm_conv_wgrad_bias', (128, 1, 1, 768, 768, 768, 768, 1, 0, -1), 'pppp')),
    ('conv-bwd', 128, 1, 1, 768, 768, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd_ws', (294912, 128, 1, 1, 768, 768, 768, 768, 768, 768, 1, 0), 'pp00pp'), ('adm_conv_wgrad_ws', (128, 1, 1, 768, 768, 768, 768, 1, 0, 1, 0), 'pppp')),
    ('conv-bwd', 128, 4, 4, 384, 1, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd', (128, 4, 4, 32, 32, 384, 384, 384, 384, 1, 0, -1), 'pp00p'), ('adm_gemm_wgrad_x6', (2048, 384, 384, 32, 32, -1), 'pppp')),
    ('conv-bwd', 128, 4, 4, 384, 1, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd', (128, 4, 4, 32, 32, 384, 384, 384, 384, 1, 0, -1), 'pp00p'), ('adm_gemm_wgrad_x6_ws', (2048, 384, 384, 32, 32, 6), 'pppp')),
    ('conv-bwd', 128, 4, 4, 384, 384, 1, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (2048, 384, 384, 384, 384, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (2048, 384, 384, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 128, 4, 4, 384, 384, 1, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (2048, 384, 384, 384, 384, 6, 1), 'pppppp'), ('adm_gemm_x6_h3', (2048, 384, 384, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 128, 4, 4, 384, 384, 3, 0, True, False, False, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (3145728, 128, 4, 4, 384, 384, 384, 384, 384, 384, 0), 'pp00ppp'), ('adm_conv_wgrad_x6', (128, 4, 4, 384, 384, 384, 384, -1), 'pppp')),
    ('conv-bwd', 128, 4, 4, 384, 384, 3, 0, True, False, False, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (3145728, 128, 4, 4, 384, 384, 384, 384, 384, 384, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_ws', (128, 4, 4, 384, 384, 384, 384, 5, 0), 'pppp')),
    ('conv-bwd', 128, 4, 4, 384, 384, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (3145728, 128, 4, 4, 384, 384, 384, 384, 384, 384, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (128, 4, 4, 384, 384, 384, 384, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 4, 4, 384, 384, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (3145728, 128, 4, 4, 384, 384, 384, 384, 384, 384, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (128, 4, 4, 384, 384, 384, 384, 5, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 4, 4, 384, 384, 3, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (3145728, 128, 4, 4, 384, 384, 384, 384, 384, 384, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (128, 4, 4, 384, 384, 384, 384, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 4, 4, 384, 384, 3, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (3145728, 128, 4, 4, 384, 384, 384, 384, 384, 384, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (128, 4, 4, 384, 384, 384, 384, 5, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 4, 4, 384, 384, 3, 1, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 8, 8, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 8, 8, 384, 384, 384, 384, -1, 1, 0), 'pppppp')),
    ('conv-bwd', 128, 4, 4, 384, 384, 3, 1, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 8, 8, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 8, 8, 384, 384, 384, 384, 7, 1, 1), 'pppppp')),
    ('conv-bwd', 128, 4, 4, 384, 1152, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (2048, 384, 384, 1152, 1152, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (2048, 1152, 1152, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 128, 4, 4, 384, 1152, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (2048, 384, 384, 1152, 1152, 2, 1), 'pppppp'), ('adm_gemm_x6_h3', (2048, 1152, 1152, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 128, 4, 4, 768, 384, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (2048, 768, 768, 384, 384, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (2048, 384, 384, 768, 768, 768, 768), 'pp00ppp')),
    ('conv-bwd', 128, 4, 4, 768, 384, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (2048, 768, 768, 384, 384, 3, 1), 'pppppp'), ('adm_gemm_x6_h3', (2048, 384, 384, 768, 768, 768, 768), 'pp00ppp')),
    ('conv-bwd', 128, 4, 4, 768, 384, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (3145728, 128, 4, 4, 384, 384, 768, 768, 768, 768, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (128, 4, 4, 768, 768, 384, 384, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 4, 4, 768, 384, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (3145728, 128, 4, 4, 384, 384, 768, 768, 768, 768, 0), 'pp00ppp'), ('adm_conv_wgrad_x6_h3', (128, 4, 4, 768, 768, 384, 384, 6, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 8, 8, 384, 384, 1, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (8192, 384, 384, 384, 384, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (8192, 384, 384, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 128, 8, 8, 384, 384, 1, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (8192, 384, 384, 384, 384, 7, 1), 'pppppp'), ('adm_gemm_x6_h3', (8192, 384, 384, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 128, 8, 8, 384, 384, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 8, 8, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 8, 8, 384, 384, 384, 384, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 8, 8, 384, 384, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 8, 8, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 8, 8, 384, 384, 384, 384, 7, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 8, 8, 384, 384, 3, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 8, 8, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 8, 8, 384, 384, 384, 384, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 8, 8, 384, 384, 3, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 8, 8, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 8, 8, 384, 384, 384, 384, 7, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 8, 8, 384, 384, 3, 1, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 384, 384, 384, 384, -1, 1, 0), 'pppppp')),
    ('conv-bwd', 128, 8, 8, 384, 384, 3, 1, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 384, 384, 384, 384, 7, 1, 1), 'pppppp')),
    ('conv-bwd', 128, 8, 8, 384, 1152, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (8192, 384, 384, 1152, 1152, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (8192, 1152, 1152, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 128, 8, 8, 384, 1152, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (8192, 384, 384, 1152, 1152, 7, 1), 'pppppp'), ('adm_gemm_x6_h3', (8192, 1152, 1152, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 128, 8, 8, 768, 384, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (8192, 768, 768, 384, 384, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (8192, 384, 384, 768, 768, 768, 768), 'pp00ppp')),
    ('conv-bwd', 128, 8, 8, 768, 384, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (8192, 768, 768, 384, 384, 7, 1), 'pppppp'), ('adm_gemm_x6_h3', (8192, 384, 384, 768, 768, 768, 768), 'pp00ppp')),
    ('conv-bwd', 128, 8, 8, 768, 384, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 8, 8, 384, 384, 768, 768, 768, 768, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 8, 8, 768, 768, 384, 384, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 8, 8, 768, 384, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 8, 8, 384, 384, 768, 768, 768, 768, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 8, 8, 768, 768, 384, 384, 8, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 192, 192, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 192, 192, 192, 192, 192, 192, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 192, 192, 192, 192, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 192, 192, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 192, 192, 192, 192, 192, 192, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 192, 192, 192, 192, 7, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 192, 192, 3, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 192, 192, 192, 192, 192, 192, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 192, 192, 192, 192, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 192, 192, 3, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 192, 192, 192, 192, 192, 192, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 192, 192, 192, 192, 7, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 192, 384, 1, 0, True, False, False, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (32768, 192, 192, 384, 384, -1), 'pppp'), ('adm_gemm_x6_h3', (32768, 384, 384, 192, 192, 192, 192), 'pp00ppp')),
    ('conv-bwd', 128, 16, 16, 192, 384, 1, 0, True, False, False, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (32768, 192, 192, 384, 384, 14), 'pppp'), ('adm_gemm_x6_h3', (32768, 384, 384, 192, 192, 192, 192), 'pp00ppp')),
    ('conv-bwd', 128, 16, 16, 192, 384, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 384, 384, 192, 192, 192, 192, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 192, 192, 384, 384, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 192, 384, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 384, 384, 192, 192, 192, 192, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 192, 192, 384, 384, 7, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 384, 384, 1, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (32768, 384, 384, 384, 384, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (32768, 384, 384, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 128, 16, 16, 384, 384, 1, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (32768, 384, 384, 384, 384, 7, 1), 'pppppp'), ('adm_gemm_x6_h3', (32768, 384, 384, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 128, 16, 16, 384, 384, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 384, 384, 384, 384, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 384, 384, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 384, 384, 384, 384, 7, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 384, 384, 3, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 384, 384, 384, 384, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 384, 384, 3, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 384, 384, 384, 384, 7, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 384, 384, 3, 1, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 32, 32, 384, 384, 384, 384, -1, 1, 0), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 384, 384, 3, 1, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 32, 32, 384, 384, 384, 384, 7, 1, 1), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 384, 1152, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (32768, 384, 384, 1152, 1152, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (32768, 1152, 1152, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 128, 16, 16, 384, 1152, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (32768, 384, 384, 1152, 1152, 7, 1), 'pppppp'), ('adm_gemm_x6_h3', (32768, 1152, 1152, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 128, 16, 16, 576, 384, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (32768, 576, 576, 384, 384, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (32768, 384, 384, 576, 576, 576, 576), 'pp00ppp')),
    ('conv-bwd', 128, 16, 16, 576, 384, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (32768, 576, 576, 384, 384, 14, 1), 'pppppp'), ('adm_gemm_x6_h3', (32768, 384, 384, 576, 576, 576, 576), 'pp00ppp')),
    ('conv-bwd', 128, 16, 16, 576, 384, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 384, 384, 576, 576, 576, 576, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 576, 576, 384, 384, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 576, 384, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 384, 384, 576, 576, 576, 576, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 576, 576, 384, 384, 13, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 768, 384, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (32768, 768, 768, 384, 384, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (32768, 384, 384, 768, 768, 768, 768), 'pp00ppp')),
    ('conv-bwd', 128, 16, 16, 768, 384, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (32768, 768, 768, 384, 384, 7, 1), 'pppppp'), ('adm_gemm_x6_h3', (32768, 384, 384, 768, 768, 768, 768), 'pp00ppp')),
    ('conv-bwd', 128, 16, 16, 768, 384, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 384, 384, 768, 768, 768, 768, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 768, 768, 384, 384, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 16, 16, 768, 384, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 16, 16, 384, 384, 768, 768, 768, 768, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 16, 16, 768, 768, 384, 384, 8, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 32, 32, 3, 192, 3, 0, True, False, True, None, True, False, False, True, True, True, True): (('adm_conv_wgrad_x6_h3', (128, 32, 32, 32, 32, 192, 192, -1, 0, 0), 'pppppp'),),
    ('conv-bwd', 128, 32, 32, 3, 192, 3, 0, True, False, True, None, True, True, False, True, True, True, True): (('adm_conv_wgrad_x6_h3', (128, 32, 32, 32, 32, 192, 192, 21, 0, 1), 'pppppp'),),
    ('conv-bwd', 128, 32, 32, 192, 3, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 32, 32, 192, 192, 192, 192, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 32, 32, 192, 192, 32, 32, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 32, 32, 192, 3, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 32, 32, 192, 192, 192, 192, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 32, 32, 192, 192, 32, 32, 21, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 32, 32, 192, 192, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 192, 192, 192, 192, 192, 192, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 32, 32, 192, 192, 192, 192, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 32, 32, 192, 192, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 192, 192, 192, 192, 192, 192, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 32, 32, 192, 192, 192, 192, 7, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 32, 32, 192, 192, 3, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 192, 192, 192, 192, 192, 192, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 32, 32, 192, 192, 192, 192, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 32, 32, 192, 192, 3, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 192, 192, 192, 192, 192, 192, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 32, 32, 192, 192, 192, 192, 7, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 32, 32, 384, 192, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (131072, 384, 384, 192, 192, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (131072, 192, 192, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 128, 32, 32, 384, 192, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (131072, 384, 384, 192, 192, 14, 1), 'pppppp'), ('adm_gemm_x6_h3', (131072, 192, 192, 384, 384, 384, 384), 'pp00ppp')),
    ('conv-bwd', 128, 32, 32, 384, 192, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 192, 192, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 32, 32, 384, 384, 192, 192, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 32, 32, 384, 192, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 192, 192, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 32, 32, 384, 384, 192, 192, 7, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 32, 32, 384, 384, 3, 0, True, True, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 32, 32, 384, 384, 384, 384, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 32, 32, 384, 384, 3, 0, True, True, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 384, 384, 384, 384, 384, 384, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 32, 32, 384, 384, 384, 384, 7, 0, 1), 'pppppp')),
    ('conv-bwd', 128, 32, 32, 576, 192, 1, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (131072, 576, 576, 192, 192, -1, 0), 'pppppp'), ('adm_gemm_x6_h3', (131072, 192, 192, 576, 576, 576, 576), 'pp00ppp')),
    ('conv-bwd', 128, 32, 32, 576, 192, 1, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_h3', (131072, 576, 576, 192, 192, 28, 1), 'pppppp'), ('adm_gemm_x6_h3', (131072, 192, 192, 576, 576, 576, 576), 'pp00ppp')),
    ('conv-bwd', 128, 32, 32, 576, 192, 3, 0, True, False, True, None, True, False, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 192, 192, 576, 576, 576, 576, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 32, 32, 576, 576, 192, 192, -1, 0, 0), 'pppppp')),
    ('conv-bwd', 128, 32, 32, 576, 192, 3, 0, True, False, True, None, True, True, True, True, True, True, True): (('adm_conv_fwd_wino2d_h3', (0, 128, 32, 32, 192, 192, 576, 576, 576, 576, 0), 'pp00p0p'), ('adm_conv_wgrad_x6_h3', (128, 32, 32, 576, 576, 192, 192, 7, 0, 1), 'pppppp')),
    ('conv-bwd', 256, 1, 1, 128, 128, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd', (256, 1, 1, 128, 128, 128, 128, 128, 128, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_bias', (256, 1, 1, 128, 128, 128, 128, 1, 0, -1), 'pppp')),
    ('conv-bwd', 256, 1, 1, 128, 128, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd', (256, 1, 1, 128, 128, 128, 128, 128, 128, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_ws', (256, 1, 1, 128, 128, 128, 128, 1, 0, 2, 0), 'pppp')),
    ('conv-bwd', 256, 1, 1, 256, 256, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd', (256, 1, 1, 256, 256, 256, 256, 256, 256, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_bias', (256, 1, 1, 256, 256, 256, 256, 1, 0, -1), 'pppp')),
    ('conv-bwd', 256, 1, 1, 256, 256, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd', (256, 1, 1, 256, 256, 256, 256, 256, 256, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_ws', (256, 1, 1, 256, 256, 256, 256, 1, 0, 2, 0), 'pppp')),
    ('conv-bwd', 256, 1, 1, 512, 512, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_conv_fwd_ws', (262144, 256, 1, 1, 512, 512, 512, 512, 512, 512, 1, 0), 'pp00pp'), ('adm_conv_wgrad_bias', (256, 1, 1, 512, 512, 512, 512, 1, 0, -1), 'pppp')),
    ('conv-bwd', 256, 1, 1, 512, 512, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_conv_fwd_ws', (262144, 256, 1, 1, 512, 512, 512, 512, 512, 512, 1, 0), 'pp00pp'), ('adm_conv_wgrad_ws', (256, 1, 1, 512, 512, 512, 512, 1, 0, 2, 0), 'pppp')),
    ('conv-bwd', 4096, 1, 1, 512, 512, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (4096, 512, 512, 512, 512, -1), 'pppp'), ('adm_gemm_x6', (4096, 512, 512, 512, 512, 512, 512), 'pp00p')),
    ('conv-bwd', 4096, 1, 1, 512, 512, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (4096, 512, 512, 512, 512, 4), 'pppp'), ('adm_gemm_x6', (4096, 512, 512, 512, 512, 512, 512), 'pp00p')),
    ('conv-bwd', 16384, 1, 1, 128, 128, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (16384, 128, 128, 128, 128, -1), 'pppp'), ('adm_gemm_x6', (16384, 128, 128, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16384, 1, 1, 128, 128, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (16384, 128, 128, 128, 128, 43), 'pppp'), ('adm_gemm_x6', (16384, 128, 128, 128, 128, 128, 128), 'pp00p')),
    ('conv-bwd', 16384, 1, 1, 256, 256, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (16384, 256, 256, 256, 256, -1), 'pppp'), ('adm_gemm_x6', (16384, 256, 256, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16384, 1, 1, 256, 256, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (16384, 256, 256, 256, 256, 16), 'pppp'), ('adm_gemm_x6', (16384, 256, 256, 256, 256, 256, 256), 'pp00p')),
    ('conv-bwd', 16384, 1, 1, 512, 512, 1, 0, True, False, False, None, False, False, True, True, True, True, True): (('adm_gemm_wgrad_x6', (16384, 512, 512, 512, 512, -1), 'pppp'), ('adm_gemm_x6', (16384, 512, 512, 512, 512, 512, 512), 'pp00p')),
    ('conv-bwd', 16384, 1, 1, 512, 512, 1, 0, True, False, False, None, False, True, True, True, True, True, True): (('adm_gemm_wgrad_x6_ws', (16384, 512, 512, 512, 512, 4), 'pppp'), ('adm_gemm_x6', (16384, 512, 512, 512, 512, 512, 512), 'pp00p')),
    ('generic', 16, 32, 32, 256, 512, 4, 2, 1, True): (('adm_conv_fwd_strided', (16, 32, 32, 16, 16, 256, 256, 512, 512, 512, 512, 4, 2, 1), 'ppp0p'),),
    ('generic', 16, 64, 64, 128, 256, 4, 2, 1, True): (('adm_conv_fwd_strided', (16, 64, 64, 32, 32, 128, 128, 256, 256, 256, 256, 4, 2, 1), 'ppp0p'),),
    ('generic', 16, 128, 128, 128, 128, 4, 2, 1, True): (('adm_conv_fwd_strided', (16, 128, 128, 64, 64, 128, 128, 128, 128, 128, 128, 4, 2, 1), 'ppp0p'),),
    ('generic', 16, 128, 128, 131, 128, 7, 1, 3, True): (('adm_conv_fwd_strided', (16, 128, 128, 128, 128, 160, 160, 128, 128, 128, 128, 7, 1, 3), 'ppp0p'),),
    ('generic-bwd', 16, 32, 32, 256, 512, 4, 2, 1, True, True, True, True): (('adm_conv_fwd', (1, 4096, 1, 512, 512, 4096, 4096, 4096, 4096, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_strided', (16, 32, 32, 16, 16, 256, 256, 512, 512, 4, 2, 1), 'pppp')),
    ('generic-bwd', 16, 64, 64, 128, 256, 4, 2, 1, True, True, True, True): (('adm_conv_fwd', (1, 16384, 1, 256, 256, 2048, 2048, 2048, 2048, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_strided', (16, 64, 64, 32, 32, 128, 128, 256, 256, 4, 2, 1), 'pppp')),
    ('generic-bwd', 16, 128, 128, 128, 128, 4, 2, 1, True, True, True, True): (('adm_conv_fwd', (1, 65536, 1, 128, 128, 2048, 2048, 2048, 2048, 1, 0, -1), 'pp00p'), ('adm_conv_wgrad_strided', (16, 128, 128, 64, 64, 128, 128, 128, 128, 4, 2, 1), 'pppp')),
    ('generic-bwd', 16, 128, 128, 131, 128, 7, 1, 3, True, False, True, True): (('adm_conv_wgrad_strided', (16, 128, 128, 128, 128, 160, 160, 128, 128, 7, 1, 3), 'pppp'),),
    ('mm', 512, 4096, 512, False): (('adm_conv_fwd', (1, 512, 1, 512, 512, 4096, 4096, 4096, 4096, 1, 0, -1), 'pp00p'),),
    ('mm', 512, 16384, 512, False): (('adm_conv_fwd', (1, 512, 1, 512, 512, 16384, 16384, 16384, 16384, 1, 0, -1), 'pp00p'),),
    ('mm', 4096, 512, 4096, True): (('adm_conv_fwd', (1, 4096, 1, 4096, 4096, 512, 512, 512, 512, 1, 0, -1), 'ppp0p'),),
    ('mm', 4096, 4096, 512, False): (('adm_conv_fwd', (1, 4096, 1, 512, 512, 4096, 4096, 4096, 4096, 1, 0, -1), 'pp00p'),),
    ('mm', 16384, 512, 16384, True): (('adm_conv_fwd', (1, 16384, 1, 16384, 16384, 512, 512, 512, 512, 1, 0, -1), 'ppp0p'),),
    ('mm', 16384, 16384, 512, False): (('adm_conv_fwd', (1, 16384, 1, 512, 512, 16384, 16384, 16384, 16384, 1, 0, -1), 'pp00p'),),
    ('strided', 2, 256, 256, 256, 256, 3, 2, 0, 1, True): (('adm_conv_fwd_strided', (2, 256, 256, 128, 128, 256, 256, 256, 256, 256, 256, 3, 2, 0), 'ppp0p'),),
    ('strided', 2, 512, 512, 128, 128, 3, 2, 0, 1, True): (('adm_conv_fwd_strided', (2, 512, 512, 256, 256, 128, 128, 128, 128, 128, 128, 3, 2, 0), 'ppp0p'),),
    ('strided', 8, 128, 128, 256, 256, 3, 2, 0, 1, True): (('adm_conv_fwd_strided', (8, 128, 128, 64, 64, 256, 256, 256, 256, 256, 256, 3, 2, 0), 'ppp0p'),),
    ('strided', 8, 256, 256, 128, 128, 3, 2, 0, 1, True): (('adm_conv_fwd_strided', (8, 256, 256, 128, 128, 128, 128, 128, 128, 128, 128, 3, 2, 0), 'ppp0p'),),
}


# ------------------------------------------------------------------------------------------------ 1: the census
@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_production_launches_are_in_the_table(ops, config, det):
    """Every launch of one training step and one sampling pass of a shipped config is in PRODUCTION_LAUNCHES."""
    pairs = census(config, det)
    print(f"census {config} ({'deterministic' if det else 'default'}): {len({k for _, k in pairs})} distinct launch keys at "
          f"{len({s for s, _ in pairs})} sites")
    missing = sorted((s, k) for s, k in pairs if k not in PRODUCTION_LAUNCHES.get(s, ()))
    assert not missing, f"{len(missing)} launches outside PRODUCTION_LAUNCHES (extend the table and the sweep), e.g. {missing[:4]}"


# ------------------------------------------------------------------------------------------------ 2: the sweep
_POOL = {}


def _hashed(shape, offset, scale, positive=False):
    """Zero-mean hashed data (oracle.fill.hash_tensor, uniform in [-scale, scale)) on the GPU: views into one hashed pool, at an offset
    per operand (hashing each production-size tensor on the host would dominate the run)."""
    if "pool" not in _POOL:
        _POOL["pool"] = fill.hash_tensor(((1 << 24) + 4099,), "acc.pool", 1.0).cuda()
    pool = _POOL["pool"]
    n = 1
    for d in shape:
        n *= d
    idx = (torch.arange(n, device="cuda", dtype=torch.int64) * 7 + offset) % pool.numel()
    t = pool[idx].reshape(shape) * scale
    return t.abs() if positive else t


def _conv_cases():
    """(forward site, backward site without its det flag or None): every conv geometry + bound / sink flags of the table."""
    bwd = {}
    for s in PRODUCTION_LAUNCHES:
        if s and s[0] == "conv-bwd":
            bwd.setdefault(("conv",) + s[1:12], set()).add(s[12:13] + s[14:])
    cases = [(f, b) for f, bs in bwd.items() for b in sorted(bs)]
    cases += [(s, None) for s in PRODUCTION_LAUNCHES if s and s[0] == "conv" and s not in bwd]
    return sorted(cases, key=lambda c: (str(c[0][11]), c[0][1:11], str(c[1])))


def _fwd_symbol(f):
    return sorted(k[0] for k in PRODUCTION_LAUNCHES[f])[0]


def _positive_cases():
    """The largest contraction (k*k*Cin) of each forward kernel family: also run on all-positive data (no cancellation)."""
    best = {}
    for f, b in _conv_cases():
        if b is None:
            continue
        fam, K = _fwd_symbol(f), f[6] * f[6] * f[4]
        if fam not in best or K > best[fam][0]:
            best[fam] = (K, f, b)
    return [(f, b) for _, f, b in sorted(best.values(), key=lambda v: v[1][1:])]


def _case_id(c):
    f, b = c
    B, H, W, ci, co, ks, up, hb, hr, hax, sel = f[1:]
    s = f"B{B}-{H}x{W}-{ci}to{co}-k{ks}{'-up' if up else ''}{'-bias' if hb else ''}{'-res' if hr else ''}{'-ax' if hax else ''}"
    s += f"-sel{sel}" if sel is not None else ""
    if b is None:
        return s + "-fwd"
    bound, ndx, ndw, ndb, wd, bd = b
    return s + f"{'-ady' if bound else ''}{'' if ndx else '-nodx'}{'-direct' if wd else ''}"


WORST = {}        # (family, path, output) -> [e_max, e_rms]


def _note(family, path, out, e):
    w = WORST.setdefault((family, path, out), [0.0, 0.0])
    w[0], w[1] = max(w[0], e[0]), max(w[1], e[1])


class _Knobs:
    """Global launcher knobs, restored in a finally by the caller."""

    def __init__(self, ops):
        from adm_amd import hip
        self.lib = hip.lib()
        self.wide = self.lib.adm_wino2d_h3_wide(-1)
        self.lib.adm_wino2d_h3_wide(self.wide)
        self.blocks = self.lib.adm_wgrad_h3_blocks(-1)
        self.lib.adm_wgrad_h3_blocks(self.blocks)

    def restore(self):
        self.lib.adm_wino2d_h3_wide(self.wide)
        self.lib.adm_wgrad_h3_blocks(self.blocks)


def _run_conv(ops, mp, rec, f, b, data, *, det=False, path="default"):
    """One forward (+ backward) of ops.conv2d at site f / b on the given data: {"y", "dx", "dw", "db": tensor} and the launches."""
    B, H, W, ci, co, ks, up, hb, hr, hax, sel = f[1:]
    x, w, bias, res, dy = data
    cip = ops.ceil32(ci)
    mp.setattr(ops, "BF16X6", path != "f32")
    mp.setattr(ops, "FP16X3", path not in ("f32", "x6"))
    mp.setattr(ops, "DETERMINISTIC", det)
    bound_dy = b is not None and b[0]
    mp.setattr(ops, "_get_amax", (lambda t: ops.amax_vector(t)) if bound_dy else (lambda t: None))
    xd = torch.zeros(B, H, W, cip, device="cuda")
    xd[..., :ci] = x
    wd = w.clone().requires_grad_(b is not None)
    bd = bias.clone().requires_grad_(b is not None and b[3]) if bias is not None else None
    if b is not None:
        xd.requires_grad_(b[1])
        for p, direct in ((wd, b[4]), (bd, b[5])):
            if p is not None and direct:       # a parameter of the flat gradient buffer: the kernels accumulate into .grad
                p.grad = torch.zeros_like(p)
                p._adm_direct = True
    rec.launches = {}
    ctx = ops.batch_invariant(sel) if sel is not None else _Null()
    with ctx:
        y = ops.conv2d(xd, wd, bd, res, up=bool(up), amax=ops.amax_vector(xd) if hax else None)
        if b is not None:
            y.backward(dy)
            ops.flush_deferred_unpack()
    torch.cuda.synchronize()
    got = {"y": y.detach()[..., :co]}
    if b is not None:
        if b[1]:
            got["dx"] = xd.grad[..., :ci]
        got["dw"] = wd.grad
        if bd is not None and b[3]:
            got["db"] = bd.grad
    return got, rec.launches


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass


def _conv_data(f, b, positive):
    B, H, W, ci, co, ks, up, hb, hr, hax, sel = f[1:]
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    cop = -(-co // 32) * 32
    x = _hashed((B, H, W, ci), 0, 1.0, positive)
    w = _hashed((co, ci, ks, ks), 1234567, (ci * ks * ks) ** -0.5, positive)
    bias = _hashed((co,), 7654321, 0.1, positive) if hb else None
    res = None
    if hr:
        res = torch.zeros(B, Ho, Wo, cop, device="cuda")
        res[..., :co] = _hashed((B, Ho, Wo, co), 3333331, 1.0, positive)
    dy = None
    if b is not None:
        dy = torch.zeros(B, Ho, Wo, cop, device="cuda")
        dy[..., :co] = _hashed((B, Ho, Wo, co), 9999991, 1.0, positive)
    return x, w, bias, res, dy


def _check_conv(ops, monkeypatch, f, b, positive):
    from adm_amd import hip
    rec = Recorder(monkeypatch)
    knobs = _Knobs(ops)
    data = _conv_data(f, b, positive)
    x, w, bias, res, dy = data
    co, ks, up = f[5], f[6], f[7]
    ref = fp64ref.conv(x, w, bias, None if res is None else res[..., :co], None if dy is None else dy[..., :co], up=bool(up))
    fam = _fwd_symbol(f)
    keys = set().union(*(PRODUCTION_LAUNCHES.get(s, ()) for s in PRODUCTION_LAUNCHES
                         if s == f or (b is not None and s[0] == "conv-bwd" and ("conv",) + s[1:12] == f and s[12:13] + s[14:] == b)))
    h3_fwd = any(k[0] == "adm_conv_fwd_wino2d_h3" for k in keys)
    h3_wgrad = any(k[0] in ("adm_conv_wgrad_x6_h3", "adm_gemm_wgrad_x6_h3") for k in keys)
    split = any(("x6" in k[0] or "h3" in k[0]) for k in keys)
    runs = [("f32", dict(path="f32"))]
    dets = (False, True) if b is not None else (False,)
    runs += [("default" + ("-det" if d else ""), dict(det=d)) for d in dets]
    if split and (h3_fwd or h3_wgrad or any("h3" in k[0] for k in keys)):
        runs.append(("x6", dict(path="x6")))
    if h3_fwd:
        runs += [(f"h3-form{v}", dict(wide=v)) for v in (0, 1, 3)]
    if h3_wgrad and b is not None:
        runs += [(f"h3-wgrad-blocks{v}" + ("-det" if d else ""), dict(blocks=v, det=d)) for v in (1, 2) for d in (False, True)]
    errs, bad = {}, []
    try:
        for name, kw in runs:
            wide, blocks = kw.pop("wide", knobs.wide), kw.pop("blocks", knobs.blocks)
            knobs.lib.adm_wino2d_h3_wide(wide)
            knobs.lib.adm_wgrad_h3_blocks(blocks)
            got, launches = _run_conv(ops, monkeypatch, rec, f, b, data, **kw)
            knobs.restore()
            if name.startswith("default"):          # the production launches come back
                det = name.endswith("-det")
                want = set(PRODUCTION_LAUNCHES.get(f, ()))
                if b is not None:
                    want |= set(PRODUCTION_LAUNCHES.get(("conv-bwd",) + f[1:] + b[:1] + (det,) + b[1:], ()))
                seen = set().union(*launches.values()) if launches else set()
                assert want <= seen, f"{name}: launches not reproduced: {sorted(want - seen)}; seen {sorted(seen)}"
            for out, t in got.items():
                assert bool(torch.isfinite(t).all()), (name, out)
                e = fp64ref.errors(t, *ref[out])
                errs[(name, out)] = e
                _note(fam if out == "y" else fam + "/" + out, "f32" if name == "f32" else name.split("-det")[0], out, e)
                if e[0] > BAR_A:
                    bad.append(f"bar A: {name} {out} e_max {e[0]:.3e} > {BAR_A}")
                if name != "f32":
                    ok, rm, rr = fp64ref.bar_b(e, errs[("f32", out)])
                    if not ok:
                        bad.append(f"bar B: {name} {out} e {e[0]:.3e}/{e[1]:.3e} vs f32 {errs[('f32', out)][0]:.3e}/"
                                   f"{errs[('f32', out)][1]:.3e} (ratios {rm:.2f}, {rr:.2f})")
    finally:
        knobs.restore()
    print(_case_id((f, b)) + (" positive" if positive else "") + ": "
          + "; ".join(f"{n}/{o} {e[0]:.1e}/{e[1]:.1e}" for (n, o), e in errs.items()))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", _conv_cases(), ids=_case_id)
def test_conv_launch_plan_vs_fp64(ops, monkeypatch, case):
    """Forward, data gradient, weight gradient and bias gradient of every production conv site against fp64 (bars A and B), on the
    default launch plan (asserted to be the recorded one), the f32-MFMA kernels, the bf16 format, every fp16-format form and every
    weight-gradient block size with the deterministic mode on and off."""
    _check_conv(ops, monkeypatch, case[0], case[1], positive=False)


@pytest.mark.parametrize("case", _positive_cases(), ids=_case_id)
def test_conv_launch_plan_vs_fp64_positive(ops, monkeypatch, case):
    """The same on all-positive data (no cancellation: the error is relative to |result|) at the largest K of each kernel family."""
    _check_conv(ops, monkeypatch, case[0], case[1], positive=True)


def _attn_cases():
    return sorted(s for s in PRODUCTION_LAUNCHES if s and s[0] == "attn-bwd")


@pytest.mark.parametrize("site", _attn_cases(), ids=lambda s: f"B{s[1]}-L{s[2]}-h{s[3]}")
def test_attention_launch_plan_vs_fp64(ops, monkeypatch, site):
    """ops.attention forward and backward at the production shapes, on the f32 kernels and on the fp16 format with bounds."""
    _, B, L, heads, hax, hdy = site
    h = int(L ** 0.5)
    rec = Recorder(monkeypatch)
    qkv = _hashed((B, h, h, heads * 192), 0, 1.0)
    dout = _hashed((B, h, h, heads * 64), 9999991, 1.0)
    ref = fp64ref.attention(qkv, heads, dout)
    errs, bad = {}, []
    for name in ("f32", "default"):
        monkeypatch.setattr(ops, "ATTN_H3", name == "default")
        monkeypatch.setattr(ops, "_get_amax", (lambda t: ops.amax_vector(t)) if (hdy and name == "default") else (lambda t: None))
        qd = qkv.clone().requires_grad_(True)
        if hax:
            qd._adm_amax = ops.amax_vector(qd)
        rec.launches = {}
        a = ops.attention(qd, heads)
        a.backward(dout)
        torch.cuda.synchronize()
        if name == "default":
            want = set(PRODUCTION_LAUNCHES[("attn",) + site[1:5]]) | set(PRODUCTION_LAUNCHES[site])
            seen = set().union(*rec.launches.values())
            assert want <= seen, (sorted(want - seen), sorted(seen))
        for out, t in (("out", a), ("dqkv", qd.grad)):
            e = fp64ref.errors(t, *ref[out])
            errs[(name, out)] = e
            _note("attention", name, out, e)
            if e[0] > BAR_A:
                bad.append(f"bar A: {name} {out} {e}")
            if name != "f32" and not fp64ref.bar_b(e, errs[("f32", out)])[0]:
                bad.append(f"bar B: {name} {out} {e} vs f32 {errs[('f32', out)]}")
    print(f"attention B={B} L={L} heads={heads}: " + "; ".join(f"{n}/{o} {e[0]:.1e}/{e[1]:.1e}" for (n, o), e in errs.items()))
    assert not bad, "\n".join(bad)


def test_zz_report_worst_errors():
    """Worst e_max / e_rms per kernel family (the forward symbol of the site; '/dx', '/dw', '/db' for its gradients) and path."""
    if not WORST:
        pytest.skip("no sweep ran in this session")
    print("\nworst error vs fp64 per family / path / output (e_max, e_rms):")
    for (fam, path, out), (em, er) in sorted(WORST.items()):
        print(f"  {fam:32s} {path:24s} {out:3s} {em:.3e} {er:.3e}")

