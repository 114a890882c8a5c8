"""Autograd operators over the HIP C ABI (libadm_hip.so).

Activations are NHWC fp32 CUDA tensors ``[B, H, W, C]`` (``[B, C]`` for the embedding path); the
channel count of every GEMM-shaped operand is padded to a multiple of 32 (3 -> 32 at the stem and
heads).  Parameters keep the reference's layouts (OIHW / [out, in]) so state_dicts interchange; the
packed GEMM operands are derived tensors cached per parameter version.

Each Function's backward is hand-written HIP as well -- autograd is only the tape.
"""
from __future__ import annotations

import ctypes
import itertools
import os
import weakref
from typing import Optional

import torch

from . import hip
from .hip import call, ptr

_f32 = torch.float32

# bench.py sets PROFILE = [] to collect (kind, algorithmic_flops, start_event, end_event) per launch of
# the GEMM-shaped kernels; events are recorded on the current stream = the stream the kernels run on.
PROFILE = None


class _Prof:
    def __init__(self, kind, flops, tag=""):
        self.kind, self.flops, self.tag = kind, flops, tag

    def __enter__(self):
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *a):
        if PROFILE is not None:
            self.e1.record()
            PROFILE.append((self.kind, self.flops, self.e0, self.e1, self.tag))


def ceil32(n: int) -> int:
    return (n + 31) // 32 * 32


def _forget(t: torch.Tensor) -> torch.Tensor:
    """A fresh allocation: a recycled address forgets the bound of its previous tenant (see _reg_amax)."""
    if _grad_amax:
        _grad_amax.pop(t.data_ptr(), None)
    return t


def _new(shape, like: torch.Tensor, dtype=_f32) -> torch.Tensor:
    return _forget(torch.empty(shape, device=like.device, dtype=dtype))


def _chk(t: torch.Tensor, name: str) -> torch.Tensor:
    hip.require_cuda(t, name)
    if t.dtype != _f32:
        raise RuntimeError(f"adm_amd: {name} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else _forget(t.contiguous())


# ------------------------------------------------------------------------------------------------
# packed-weight cache
# ------------------------------------------------------------------------------------------------
# One row of adm_pack_weight_table: the column indices (the same names are the enum of csrc/pack_weights.hip; include/adm_hip.h says what
# each column holds) ...
(PT_SRC, PT_FWD, PT_BWD, PT_CO, PT_CI, PT_TAPS, PT_CO_PAD, PT_CI_PAD, PT_QKV, PT_TILE_BEGIN, PT_WF, PT_WB, PT_W2F, PT_W2B, PT_W2F6, PT_W2B6,
 PT_G6F, PT_G6B, PT_W2FH, PT_W2BH, PT_H3_SCALE, PT_H3_FLAG, PT_G6FH, PT_G6BH) = range(24)
PACK_TABLE_COLS = 24        # = PT_COLS of csrc/pack_weights.hip
# ... and the derived weight images of a packed entry that repack_all() keeps current, each with its column.  All are built on first use
# (_image), so most are None for most layers.
_PACK_IMAGES = (("wf", PT_WF), ("wb", PT_WB),              # 1-D Winograd operands (conv_wino.hip)
                ("w2f", PT_W2F), ("w2b", PT_W2B),          # 2-D Winograd planes, f32 (conv_wino2d.hip)
                ("w2f6", PT_W2F6), ("w2b6", PT_W2B6),      # ... their three-term bf16 splits (conv_wino2d_x6.hip)
                ("w2fh", PT_W2FH), ("w2bh", PT_W2BH),      # ... their two-term fp16 images
                ("g6f", PT_G6F), ("g6b", PT_G6B),          # three-term bf16 splits of the 1x1 operands (conv_gemm_x6.hip)
                ("g6fh", PT_G6FH), ("g6bh", PT_G6BH))      # ... their two-term fp16 images
_H3_IMAGES = ("w2fh", "w2bh", "g6fh", "g6bh")              # the images that can overflow: their rows carry the device flag


class _Packed:
    """The f32 operands `fwd` / `bwd` are refreshed ON DEMAND: most layers run on the split kernels, which read the 16-bit images, and
    would have both f32 operands rewritten by every repack without anyone reading them.  Reading the attribute is the use:
    repack_all() refreshes, in its one launch, the operands that were read since the previous repack and leaves the others stale;
    the next read of a stale operand refreshes that one with a per-layer adm_pack_weight launch (on the reader's stream) and brings
    it back into the table.  A layer on the direct kernels reads every step, so it never leaves the table.  Bookkeeping goes around
    the properties: the raw slots `_fwd` / `_bwd`, or _operand(ent, which, count=False) for a one-time read that needs current values."""
    __slots__ = (("key", "_fwd", "_bwd", "bias", "fwd16", "bwd16", "src", "h3_off", "_read", "_stale", "_owner")
                 + tuple(name for name, _ in _PACK_IMAGES))

    def __init__(self):
        for name in self.__slots__:
            setattr(self, name, None)
        self.h3_off = False          # True: a fp16 image of this entry overflowed (_h3_weight_image), the layer stays on the bf16 format
        self._read = 3               # bit 0 / 1: fwd / bwd was read since the last repack (an entry made by hand: always refreshed)
        self._stale = 0              # bit 0 / 1: fwd / bwd was left out of the last repack(s)

    fwd = property(lambda self: _operand(self, 0), lambda self, t: setattr(self, "_fwd", t))
    bwd = property(lambda self: _operand(self, 1), lambda self, t: setattr(self, "_bwd", t))


operand_refreshes = 0       # diagnostics: per-layer launches that refreshed a stale f32 operand (none in a steady training loop)


def _operand(ent: "_Packed", which: int, count: bool = True):
    """The current f32 operand of a packed entry: which = 0 forward, 1 data gradient (the properties _Packed.fwd / .bwd).  count=False:
    a one-time read (the source of an image's first build) that must not keep the operand in the repack table."""
    global operand_refreshes
    bit = 1 << which
    if ent._stale & bit:
        w = ent._owner() if ent._owner is not None else None
        if w is None:
            raise RuntimeError("adm_amd: a packed operand outlived its parameter")
        co, ci, ks, qkv = ent.src
        w = _chk(w.detach(), "weight")
        call("adm_pack_weight", ptr(w), None if which else ptr(ent._fwd), ptr(ent._bwd) if which else None, co, ci, ks, ceil32(co),
             ceil32(ci), int(qkv))
        ent._stale &= ~bit
        operand_refreshes += 1
    if count:
        ent._read |= bit
    return ent._bwd if which else ent._fwd


# Contraction precision of the conv / Linear kernels: "f32" (default: exact fp32 MFMA) or "bf16" (BASELINE
# configs[2]: bf16 MFMA operands, fp32 accumulation and storage).  Opt-in only; see set_compute_precision().
COMPUTE = "f32"

# 3x3 stride-1 convs (forward and data gradient) with M >= WINO_MIN_M output pixels and an even width run through the
# 1-D Winograd F(2,3) kernel (adm_conv_fwd_wino: 1.5x fewer MFMA flops, fp32, error at the direct kernel's own rounding
# level).  ADM_WINOGRAD=0 keeps every conv on the direct implicit GEMM.
WINOGRAD = os.environ.get("ADM_WINOGRAD", "1") != "0"
# 2048 = the 4x4 maps of the CIFAR UNet at bs=128 included: 100-143 TFLOP/s on the split-bf16 kernels against 78-105 on the direct f32
# kernels, 7.65 -> 6.2 ms per step (round 2 parked this at 8192 because the choice then differs between a batch and its chunks at small
# sizes; callers that split a batch into passes and need identical bits now say so: batch_invariant() below).
WINO_MIN_M = int(os.environ.get("ADM_WINO_MIN_M", "2048"))
# ... and those with an even height too (not the fused nearest-x2 ones) through the 2-D F(2x2, 3x3) kernel (adm_conv_fwd_wino2d:
# 2.25x fewer MFMA flops than the direct kernel).  ADM_WINOGRAD2D=0 keeps them on the 1-D kernel.
WINOGRAD2D = os.environ.get("ADM_WINOGRAD2D", "1") != "0"
# ... with their f32 products carried on the bf16 MFMA through the EXACT three-term bf16 split of both operands (conv_wino2d_x6.hip:
# six bf16 MFMAs per product block, f32 accumulation; error against fp64 at or below the f32 MFMA kernel's, see
# tests/test_hip_ops.py::test_conv_x6_error_vs_fp64).  ADM_BF16X6=0 keeps the f32-MFMA kernels of conv_wino2d.hip.
BF16X6 = os.environ.get("ADM_BF16X6", "1") != "0"
# ... or, where the activation operand comes with an upper bound of its magnitude (a GroupNorm output: the GroupNorm kernel writes
# max |y| next to it), on THREE fp16 MFMAs per product: two-term round-to-nearest split after a power-of-two scaling (conv_wino2d_x6.hip,
# X6Fmt<1>).  Same error against fp64 as the six-bf16 form (tools/fp16x3_accuracy.py, tests/test_hip_ops.py::test_conv_h3_*), half its
# matrix, LDS and split work.  Weights use one fixed power-of-two scale (H3_WSCALE = 2^11): a Winograd-domain 3x3 weight or a 1x1 weight
# >= 32 leaves the fp16 range.  Each fp16 weight image is checked when it is built (first use, and again after load_state_dict or any
# other change of the parameter made a new packed entry: one 4-byte read-back per build, _h3_weight_image): a layer whose image
# overflows keeps running on the bf16 format.  Weights that only GROW past the limit during training (the images are then rewritten
# in place by repack_all()) raise a device flag that repack_all() reads every 64 steps and that switches the format off everywhere.
# ADM_FP16X3=0 keeps every split kernel on the bf16 format.
FP16X3 = os.environ.get("ADM_FP16X3", "1") != "0"
H3_WGRAD = os.environ.get("ADM_FP16X3_WGRAD", "1") != "0"      # ... also for the weight gradients
H3_GEMM = os.environ.get("ADM_FP16X3_GEMM", "1") != "0"        # ... and for the 1x1 convs (conv_gemm_x6.hip FMT 1), which takes bounds of conv / attention / concat OUTPUTS
H3_WSCALE = 2048.0
_h3_flag = None             # device int32: raised by the weight split kernels on overflow
_h3_checks = 0
_amax_pool, _amax_next = None, 0
_amax_pool_captured, _amax_pool_size = False, 0
_AMAX_POOL = 4096


def _fp16_format() -> bool:
    """The fp16 split format is on: kernels that can write max |output| next to their output do, and consumers that find a bound on
    their operand use it.  Read at call time (tests switch the three); the 1x1 convs and what feeds them also ask for H3_GEMM."""
    return FP16X3 and BF16X6 and COMPUTE == "f32"


AMAX_FLOATS = 64 * 32      # a bound vector: ADM_AMAX_SLOTS floats at a stride of ADM_AMAX_STRIDE (include/adm_hip.h)


def _amax_slot(like: torch.Tensor) -> torch.Tensor:
    """A zeroed BOUND VECTOR (include/adm_hip.h: 64 floats, one cache line apart; the bound is their maximum) for a kernel to raise to
    max |output| -- every wave raises its own slot: one address for all of them serialised the atomics of a launch (185 us for
    a 22 us add3).  Vectors come from a pool that is zero-filled once per 4096 vectors (no per-call fill launch); a vector lives as
    long as a tensor refers to it.  The pool is filled on whichever stream asks for the vector that needs a new pool (the main, the
    second decoder's or the weight-gradient side stream): _bound_use() orders every other stream that touches it after that fill."""
    global _amax_pool, _amax_next, _amax_pool_captured, _amax_pool_size
    # Under HIP-graph capture (the sampler's replayed forward) the pool is allocated INSIDE the capture, so that its zero fill is part
    # of the graph and every replay starts from zeroed vectors: bounds never carry over from an earlier replay (a larger stale bound
    # would only change the scale by a power of two -- but replays are promised bit-identical to eager launches).
    capturing = like.is_cuda and torch.cuda.is_current_stream_capturing()
    if (_amax_pool is None or _amax_next >= _amax_pool_size or _amax_pool.device != like.device
            or capturing != _amax_pool_captured):
        _amax_pool_size = 1024 if capturing else _AMAX_POOL
        _amax_pool, _amax_next = torch.zeros(_amax_pool_size * AMAX_FLOATS, device=like.device, dtype=_f32), 0
        _amax_pool_captured = capturing
        if like.is_cuda:
            cur = torch.cuda.current_stream(like.device)
            _amax_pool._adm_users = {cur.cuda_stream}      # streams ordered after the fill and holding a lifetime mark
            if not capturing:
                _amax_pool._adm_fill = torch.cuda.Event()
                _amax_pool._adm_fill.record(cur)
    s = _amax_pool[_amax_next * AMAX_FLOATS:(_amax_next + 1) * AMAX_FLOATS]
    _amax_next += 1
    return _bound_use(s)


def _bound_use(v):
    """A kernel on the current stream is about to raise or read the bound vector v.  The first time a stream touches a pool, it waits
    for the pool's zero fill (an event on the stream that filled it) and marks the pool as used by it (record_stream), so that the
    allocator does not hand the pool's memory out again while that stream may still read or raise a bound in it: the side stream's
    weight gradients read the bounds of x and dy, the second decoder's stream raises and reads bounds of pools another stream filled.
    Once per pool and stream."""
    if v is None or not v.is_cuda:
        return v
    pool = v if v._base is None else v._base
    users = getattr(pool, "_adm_users", None)
    if users is None:                 # a vector made outside the pools (amax_vector): its lifetime is all that needs a mark
        users = pool._adm_users = set()
    s = torch.cuda.current_stream(v.device)
    if s.cuda_stream not in users:
        if torch.cuda.is_current_stream_capturing():
            return v
        fill = getattr(pool, "_adm_fill", None)
        if fill is not None:
            s.wait_event(fill)
        pool.record_stream(s)
        users.add(s.cuda_stream)
    return v


def _bptr(v):
    """ptr() of a bound vector that a kernel on the current stream reads (see _bound_use)."""
    return ptr(_bound_use(v))


def _check_bound(t: torch.Tensor, v, what: str):
    """AMAX_CHECK: the bound vector v must be >= max |t| (one host read each: tests only)."""
    if AMAX_CHECK and v is not None:
        got, bound = float(t.detach().abs().max()), float(v.max())
        if not got <= bound:
            raise RuntimeError(f"adm_amd: the bound {bound} of {what} is below its maximum {got}")


def new_amax_pool():
    """The next bound vector comes from a fresh pool (HIP-graph capture: ddm/ddpm.py)."""
    global _amax_pool
    _amax_pool = None


def amax_vector(t: torch.Tensor, loose: float = 1.0) -> torch.Tensor:
    """The bound vector of a tensor computed the slow way (tests, tools): max |t| x loose in slot 0, zeros elsewhere."""
    v = torch.zeros(AMAX_FLOATS, device=t.device, dtype=_f32)
    v[0] = t.detach().abs().max().to(_f32) * loose
    return v


# Bounds of GRADIENT tensors travel by address: autograd hands a backward node new Python objects for its incoming gradients, so an
# attribute set by the producing node does not arrive.  The producing node registers (address -> slot, numel, pass id); the consuming
# conv looks its dy up; every allocation through _new() / _like() forgets the address it returns (a recycled address must not meet
# the bound of its previous tenant), and entries of an earlier backward pass are ignored.  Each entry also keeps the tensor's version:
# a gradient that was modified after it was registered (autograd sums the gradients of a tensor with two consumers IN PLACE into the
# first one's buffer unless ops.fanout() does the sum) is no longer covered by that bound, and the lookup then finds none.
_grad_amax = {}


def _reg_amax(t: torch.Tensor, slot):
    if slot is not None:
        tid = _graph_task_id()
        if len(_grad_amax) > 8192:       # forget the entries of earlier backward passes (never this pass's: their consumers are still to come)
            for k in [k for k, e in _grad_amax.items() if e[2] != tid]:
                del _grad_amax[k]
        _grad_amax[t.data_ptr()] = (slot, t.numel(), tid, t._version)


def _get_amax(t: torch.Tensor):
    e = _grad_amax.get(t.data_ptr())
    if e is not None and e[1] == t.numel() and e[2] == _graph_task_id() and e[2] >= 0 and e[3] == t._version:
        _check_bound(t, e[0], "a gradient tensor (registered)")
        return e[0]
    return None


AMAX_CHECK = os.environ.get("ADM_AMAX_CHECK", "0") == "1"      # tests: verify every registered bound against the tensor it came with


def _like(x: torch.Tensor) -> torch.Tensor:
    return _forget(torch.empty_like(x))


def _h3_flag_tensor(like):
    global _h3_flag
    if _h3_flag is None or _h3_flag.device != like.device:
        _h3_flag = torch.zeros(1, device=like.device, dtype=torch.int32)
    return _h3_flag


def _h3_weight_image(ent: "_Packed", split) -> bool:
    """Runs split(flag) -- a weight split kernel that raises the int32 device flag it is given when a scaled weight leaves the fp16
    range -- on a fresh flag and reads it back: False (and the entry is marked to stay on the bf16 format) when the image overflowed."""
    flag = torch.zeros(1, device=ent._fwd.device, dtype=torch.int32)
    split(flag)
    if torch.cuda.is_current_stream_capturing():     # (no read-back inside a capture: the sampler packs in its eager warm-up first)
        return True
    if int(flag) != 0:
        ent.h3_off = True
        return False
    return True


def _invalidate_pack_table():
    """The one-launch repack table (repack_all) must be rebuilt: a destination was added, dropped or moved."""
    global _pack_table
    _pack_table = None


def _image(ent: "_Packed", names: tuple, build):
    """The derived image in the first of the slots `names` of a packed entry (slots that one kernel fills together).  Empty slots are
    built on first use -- build() returns one tensor per slot, or None when the image cannot be had -- and stored, and the repack table
    is invalidated so that repack_all() refreshes the new destinations from then on.  (The builders look at their slot before they come
    here: they run on the host path of every conv launch, where the call and build's closure cost more than the lookup.)"""
    if getattr(ent, names[0]) is None:
        made = build()
        if made is None:
            return None
        for name, t in zip(names, made):
            setattr(ent, name, t)
        _invalidate_pack_table()
    return getattr(ent, names[0])


def _wino2_planes(weight: torch.Tensor):
    """(forward, data-gradient) f32 2-D Winograd planes G g G^T of a 3x3 weight: [16][cop][cip], [16][cip][cop]."""
    co, ci = weight.shape[0], weight.shape[1]
    cop, cip = ceil32(co), ceil32(ci)
    w = _chk(weight.detach(), "weight")
    w2f, w2b = _new((16, cop, cip), w), _new((16, cip, cop), w)
    call("adm_pack_weight_wino2d", ptr(w), ptr(w2f), ptr(w2b), co, ci, cop, cip)
    return w2f, w2b


def _h3_operands(weight: torch.Tensor, ent: "_Packed", which: int):
    """fp16-format image of a 2-D Winograd operand (which = 0: forward, 1: data gradient), built on first use from the f32 planes and
    afterwards refreshed by repack_all() with the rest.  Only the direction that is asked for is built and kept current: most layers
    never need the other format's image of the same direction (a third of the repack table's bytes).  None when the layer's weights
    do not fit the fp16 image (the caller runs the bf16 format)."""
    if ent.h3_off:
        return None
    name = "w2bh" if which else "w2fh"
    if getattr(ent, name) is not None:
        return getattr(ent, name)

    def build():
        src = _wino2_planes(weight)[which]
        rows, cols = src.shape[1], src.shape[2]
        img = torch.empty((16, 2, rows, cols), device=src.device, dtype=torch.float16)
        ok = _h3_weight_image(ent, lambda flag: call("adm_split2_f16", ptr(src), ptr(img), rows, cols, H3_WSCALE, ptr(flag)))
        return (img,) if ok else None
    return _image(ent, (name,), build)


# ADM_DETERMINISTIC=1: bitwise reproducible backward.  The weight / bias gradient kernels normally combine their pixel-range
# splits with fp32 atomics (order-dependent rounding); with this switch every split stores its partial tile to a workspace
# and the unpack launch sums them in split order (_wgrad_workspace / _unpack_wgrad below).  Everything else on the
# training step (forward, data gradients, GroupNorm, attention, loss, norm, optimiser) is reproducible unconditionally.
DETERMINISTIC = os.environ.get("ADM_DETERMINISTIC", "0") == "1"


# In the bf16 mode the GroupNorm(+SiLU+dropout) outputs that feed a conv are STORED as bf16 in HBM (BASELINE configs[2]: "bf16
# activations"): adm_gn_fwd_bf16out writes them, adm_conv_fwd_bf16a / adm_conv_wgrad_bf16a read them directly (half the bytes, no
# conversion pass; bit-identical to rounding on load).  The residual stream, statistics, gradients and master weights stay f32.
BF16_STORAGE = os.environ.get("ADM_BF16_STORAGE", "1") != "0"


# Callers that run ONE logical batch as several passes (the frozen autoencoder's <= 1 GiB chunks) need every image to get the same
# bits whatever the chunking.  Kernel selection and split-K both look at the number of pixels in the call, so inside
# `with batch_invariant(B_total):` the selection uses the whole batch's size and the split-K variants (whose split count depends on
# the call's size) are not taken.
_SELECT_BATCH = None


class batch_invariant:
    def __init__(self, total_batch: int):
        self.total = int(total_batch)

    def __enter__(self):
        global _SELECT_BATCH
        self.old, _SELECT_BATCH = _SELECT_BATCH, self.total
        return self

    def __exit__(self, *a):
        global _SELECT_BATCH
        _SELECT_BATCH = self.old


def _sel_batch(B: int) -> int:
    return B if _SELECT_BATCH is None else max(B, _SELECT_BATCH)


def bf16_storage() -> bool:
    return COMPUTE == "bf16" and BF16_STORAGE


def set_compute_precision(mode: str):
    global COMPUTE
    if mode not in ("f32", "bf16"):
        raise ValueError("compute precision must be 'f32' or 'bf16'")
    COMPUTE = mode


def _bf16_operand(ent: "_Packed", which: str) -> torch.Tensor:
    """bf16 copy of a packed weight operand, built on first use per packed entry (no row of the repack table: repack_all() drops it)."""
    name = which + "16"
    t = getattr(ent, name)
    if t is None:
        src = getattr(ent, which)
        t = torch.empty(src.shape, device=src.device, dtype=torch.bfloat16)
        call("adm_f32_to_bf16", ptr(src), ptr(t), src.numel())
        setattr(ent, name, t)
    return t


def _wino_operands(weight: torch.Tensor, ent: "_Packed"):
    """Winograd operands (G g) of a packed 3x3 entry, built on first use; afterwards refreshed by repack_all()."""
    def build():
        co, ci = weight.shape[0], weight.shape[1]
        cop, cip = ceil32(co), ceil32(ci)
        w = _chk(weight.detach(), "weight")
        wf, wb = _new((4, cop, 3, cip), w), _new((4, cip, 3, cop), w)
        call("adm_pack_weight_wino", ptr(w), ptr(wf), ptr(wb), co, ci, cop, cip)
        return wf, wb
    if ent.wf is None:
        _image(ent, ("wf", "wb"), build)
    return ent.wf, ent.wb


def _wino2_operands(weight: torch.Tensor, ent: "_Packed", which: int):
    """2-D Winograd operand (G g G^T, 16 planes) of a packed 3x3 entry for the forward (which = 0) or the data gradient (1), built on
    first use; refreshed by repack_all().  With BF16X6 only the three-term bf16 split of the direction that is asked for is built
    and kept (conv_wino2d_x6.hip reads nothing else): the f32 planes, and the image of a direction that runs on the fp16 format,
    would be rewritten by every repack without ever being read."""
    if not BF16X6:
        if ent.w2f is None:
            _image(ent, ("w2f", "w2b"), lambda: _wino2_planes(weight))
        return ent.w2b if which else ent.w2f
    name = "w2b6" if which else "w2f6"
    if getattr(ent, name) is not None and ent.w2f is None:
        return getattr(ent, name)

    def build():
        src = (ent.w2b if which else ent.w2f) if ent.w2f is not None else _wino2_planes(weight)[which]
        img = torch.empty((16, 3) + tuple(src.shape[1:]), device=src.device, dtype=torch.bfloat16)
        call("adm_split3_bf16", ptr(src), ptr(img), src.shape[1], src.shape[2])     # K-chunk-tiled: a = a0 + a1 + a2 exactly
        return (img,)
    img = _image(ent, (name,), build)
    if ent.w2f is not None:          # (left from a run with BF16X6 off)
        ent.w2f = ent.w2b = None
        _invalidate_pack_table()
    return img


GEMM_X6_MIN_M = int(os.environ.get("ADM_GEMM_X6_MIN_M", "2048"))      # (8192 until round 3: the 4x4 level's 1x1 convs, +0.7 %)
# The 1x1 WEIGHT gradient on the split-bf16 kernel (conv_wgrad_x6.hip MODE 1: four 16-pixel chunks in place of the four ex planes).
# With the first version of that kernel it was no faster than the f32 direct kernel (65-103 vs 47-111 TFLOP/s per shape); on the
# twelve-wave version (one plane per consumer wave, 64 x 64 tiles) it is: 84-126 vs 51-109 TFLOP/s on every 1x1 shape of the UNet
# with >= 8192 pixels, 9.2 -> 7.8 ms per step.  ADM_GEMM_WGRAD_X6=0 -> the f32 kernel.
GEMM_WGRAD_X6 = os.environ.get("ADM_GEMM_WGRAD_X6", "1") == "1"


def _use_gemm_x6(M: int, ks: int, up, n_p: int, k_p: int) -> bool:
    """1x1 convs with many pixels run on conv_gemm_x6.hip (f32 products on the bf16 MFMA, exact three-term split)."""
    # (128-cout workgroup tiles: a ragged last tile reads zero weight rows and stores nothing -- 192 couts pay a quarter of padding and
    #  are still well ahead of the f32 direct kernel: the 32x32 level's skip convs, 2.8 -> 1.6 ms per step)
    return BF16X6 and ks == 1 and not up and M >= GEMM_X6_MIN_M and n_p >= 128 and k_p % 32 == 0


def _gemm_x6_operand(ent: "_Packed", which: int):
    """[K/16][3][rows][16] bf16 image of a packed 1x1 operand (which = 0 forward: rows = couts; 1 data gradient: rows = cins), built on
    first use (only the direction that is asked for), refreshed by repack_all() afterwards."""
    name = "g6b" if which else "g6f"
    if getattr(ent, name) is not None:
        return getattr(ent, name)

    def build():
        src = _operand(ent, which, count=False)      # (a one-time read: it does not keep the f32 operand in the repack table)
        img = torch.empty((3,) + tuple(src.shape), device=src.device, dtype=torch.bfloat16)
        call("adm_split3_rows", ptr(src), ptr(img), src.shape[0], src.shape[1], src.shape[1])
        return (img,)
    return _image(ent, (name,), build)


def _gemm_h3_operand(ent: "_Packed", which: int):
    """[K/16][2][rows][16] fp16 image (scale H3_WSCALE) of a packed 1x1 operand: which = 0 forward (rows = couts), 1 data gradient (rows =
    cins); built on first use, refreshed by repack_all() afterwards; None when the weights do not fit it (see _h3_weight_image)."""
    if ent.h3_off:
        return None
    name = "g6bh" if which else "g6fh"
    if getattr(ent, name) is not None:
        return getattr(ent, name)

    def build():
        src = _operand(ent, which, count=False)      # (a one-time read: it does not keep the f32 operand in the repack table)
        img = torch.empty((2,) + tuple(src.shape), device=src.device, dtype=torch.float16)
        ok = _h3_weight_image(ent, lambda flag: call("adm_split2_rows_f16", ptr(src), ptr(img), src.shape[0], src.shape[1], src.shape[1],
                                                     H3_WSCALE, ptr(flag)))
        return (img,) if ok else None
    return _image(ent, (name,), build)


_pack_epoch = 0     # bumped by code that rewrites parameters through raw pointers (fused optimiser)


def packed(weight: torch.Tensor, bias: Optional[torch.Tensor], ks: int, qkv: bool) -> _Packed:
    """(wp_fwd, wp_bwd, bias_packed) for an OIHW / [out,in] parameter.  The entry lives ON the
    parameter object (so it dies with it -- no global table that a recycled device address could
    alias) and is rebuilt when the parameter's storage or version changed (in-place updates bump
    ``_version``; the fused optimiser, which writes through raw pointers, calls invalidate_packed())."""
    co, ci = weight.shape[0], weight.shape[1]
    cop, cip = ceil32(co), ceil32(ci)
    key = (weight.data_ptr(), weight._version, _pack_epoch, ks, qkv,
           None if bias is None else (bias.data_ptr(), bias._version))
    ent = getattr(weight, "_adm_packed", None)
    if ent is not None and ent.key == key:
        return ent
    w = _chk(weight.detach(), "weight")
    ent = _Packed()
    ent.key = key
    ent.src = (co, ci, ks, qkv)
    ent._fwd = _new((cop, ks * ks * cip), w)
    ent._bwd = _new((cip, ks * ks * cop), w)
    ent._read, ent._owner = 0, weakref.ref(weight)      # both current and not read yet (see _Packed)
    call("adm_pack_weight", ptr(w), ptr(ent._fwd), ptr(ent._bwd), co, ci, ks, cop, cip, int(qkv))
    if bias is not None and not qkv and cop == co:
        ent.bias = _chk(bias.detach(), "bias")          # usable as is
    elif bias is not None:
        b = _chk(bias.detach(), "bias")
        ent.bias = _new((cop,), w)
        call("adm_permute_vec", ptr(b), ptr(ent.bias), co, cop, int(qkv), 0)
    try:
        weight._adm_packed = ent
        # only PARAMETERS join the one-launch repack table: a derived weight (weight standardisation: a fresh tensor per step)
        # would only churn it
        if isinstance(weight, torch.nn.Parameter):
            _pack_registry[id(weight)] = (weakref.ref(weight), None if bias is None else weakref.ref(bias), ks, qkv)
            _invalidate_pack_table()
    except (AttributeError, TypeError):
        pass
    return ent


def invalidate_packed():
    global _pack_epoch
    _pack_epoch += 1


# Registry of live packed parameters, so that the optimiser can refresh ALL packed operands with one launch
# (adm_pack_weight_table) instead of two small launches per layer on first use after every step.
_pack_registry: dict = {}
_pack_table = None          # (device int64 table, [entries], total 32x32 tiles, host rows, the entries' _read masks the table was made for)
pack_table_builds = 0       # diagnostics: uploads of that table (a blocking copy: none in a steady training loop)


_H3_WSCALE_BITS = int.from_bytes(__import__("struct").pack("<f", H3_WSCALE), "little")


def _pack_row(src: torch.Tensor, ent: _Packed, co: int, ci: int, ks: int, qkv: bool, tile_begin: int) -> list:
    """The row of adm_pack_weight_table that re-derives every operand of the packed entry `ent` from the OIHW / [out, in] tensor `src`:
    fwd, bwd and whichever images exist (_PACK_IMAGES); tile_begin = the 32 x 32 tiles of the rows before this one.  (Always both f32
    operands: repack_all() zeroes the column of one that nobody read.)"""
    row = [0] * PACK_TABLE_COLS
    row[PT_SRC], row[PT_FWD], row[PT_BWD] = src.data_ptr(), ent._fwd.data_ptr(), ent._bwd.data_ptr()
    row[PT_CO], row[PT_CI], row[PT_TAPS], row[PT_CO_PAD], row[PT_CI_PAD] = co, ci, ks * ks, ceil32(co), ceil32(ci)
    row[PT_QKV], row[PT_TILE_BEGIN] = int(qkv), tile_begin
    for name, col in _PACK_IMAGES:
        img = getattr(ent, name)
        if img is not None:
            row[col] = img.data_ptr()
    row[PT_H3_SCALE] = _H3_WSCALE_BITS
    if any(getattr(ent, name) is not None for name in _H3_IMAGES):      # an image that leaves the fp16 range raises the device flag
        row[PT_H3_FLAG] = _h3_flag_tensor(src).data_ptr()
    return row


def repack_all():
    """Called by the fused optimiser after it rewrote the flat parameter buffer: re-derives every registered packed
    operand in place with one kernel launch and marks the entries current.  Of the f32 operands only those that were read since the
    previous repack are refreshed (_Packed); the device table is rebuilt when that set changes."""
    global _pack_table, _pack_epoch, _h3_checks, FP16X3, pack_table_builds
    _pack_epoch += 1
    if _h3_flag is not None and FP16X3:
        _h3_checks += 1
        if _h3_checks % 64 == 0 and int(_h3_flag) != 0:      # (one 4-byte read-back per 64 optimiser steps)
            FP16X3 = False
            print("adm_amd: a Winograd-domain weight left the fp16 range at scale 2^11: the split kernels continue on the bf16 format",
                  flush=True)
    if _pack_table is None:
        rows, ents, tiles = [], [], 0
        for key, (wref, bref, ks, qkv) in list(_pack_registry.items()):
            w = wref()
            ent = getattr(w, "_adm_packed", None) if w is not None else None
            if w is None or ent is None or not w.is_cuda:
                _pack_registry.pop(key, None)
                continue
            co, ci = w.shape[0], w.shape[1]
            rows.append(_pack_row(w, ent, co, ci, ks, qkv, tiles))
            tiles += (ceil32(co) // 32) * (ceil32(ci) // 32)       # PT_TILE_BEGIN = exclusive prefix sum of 32x32 tiles
            ents.append((wref, bref, ks, qkv, ent))
        if not rows:
            return
        _pack_table = (None, ents, tiles, rows, None)
    table, ents, total_tiles, rows, masks = _pack_table
    for (wref, bref, ks, qkv, ent), row in zip(ents, rows):      # storage moved or parameter died -> rebuild lazily
        w = wref()
        if w is None or w.data_ptr() != row[PT_SRC] or getattr(w, "_adm_packed", None) is not ent:
            _pack_table = None
            return
    read = tuple(e[4]._read for e in ents)
    if table is None or read != masks:
        masked = [row if m == 3 else row[:PT_FWD] + [row[PT_FWD] * (m & 1), row[PT_BWD] * (m >> 1)] + row[PT_BWD + 1:]
                  for row, m in zip(rows, read)]
        table = torch.tensor(masked, dtype=torch.int64, device=ents[0][0]().device)
        _pack_table = (table, ents, total_tiles, rows, read)
        pack_table_builds += 1
    call("adm_pack_weight_table", ptr(table), len(ents), total_tiles)
    for (wref, bref, ks, qkv, ent), m in zip(ents, read):
        ent._stale |= 3 & ~m
        ent._read = 0
        w = wref()
        b = bref() if bref is not None else None
        co = w.shape[0]
        if b is not None and (qkv or ceil32(co) != co):
            call("adm_permute_vec", ptr(b.detach()), ptr(ent.bias), co, ceil32(co), int(qkv), 0)
        ent.fwd16 = ent.bwd16 = None
        ent.key = (w.data_ptr(), w._version, _pack_epoch, ks, qkv, None if b is None else (b.data_ptr(), b._version))


# ------------------------------------------------------------------------------------------------
# deferred weight-gradient unpack (launches per step)
# ------------------------------------------------------------------------------------------------
# The weight-gradient kernels leave a packed (and, for the 2-D Winograd form, half-transformed) tile per layer; a small "unpack"
# launch per layer used to scatter it into the flat gradient buffer, and a memset per layer cleared the tile before the split-K
# atomics.  With direct gradients (adm_amd.optim.FlatParams) both go away: every layer owns a persistent workspace that is ZERO AT
# REST, the kernels are told so (splits = -1: no memset), and ONE adm_unpack_wgrad_table launch at the end of the backward pass
# scatters all layers and clears what it read.  A gradient sink (the bucketed DDP reducer) needs the gradient when it is
# notified, so any notification flushes first.  ADM_DEFER_UNPACK=0 restores the per-layer launches.
DEFER_UNPACK = os.environ.get("ADM_DEFER_UNPACK", "1") != "0"
_UT_ITEMS = 2048            # gradient elements per workgroup of adm_unpack_wgrad_table
_TABLE_CACHE = 256          # row sets kept per table cache
_rest_ws = {}               # (weight data_ptr, shape) -> zero-at-rest workspace
# pending weight-gradient rows (host ints; the last entry of a row = its block count), the tensors they point into, and the workspaces
# among them: a layer applied twice in one pass must not meet its own pending tile
_unpack_rows, _unpack_keep, _unpack_pending = [], [], set()
# ... and the pending GroupNorm parameter-gradient reductions (tot, ss, bstride, dgamma, dbeta, B, C, blocks), with their dgamma destinations
_gn_rows, _gn_keep, _gn_pending = [], [], set()
_unpack_tables = {}         # row set -> (device table, total blocks)
_gn_tables = {}             # ... the same: with a bucketed reducer every bucket flushes its own set, every step
_pinned_tables = []         # host copies of uploaded tables (pinned: the copy is asynchronous; kept alive with the cache)
table_uploads = 0           # diagnostics: host->device table copies (asynchronous, from pinned memory)
_producer_streams = {}      # streams on which queued work was produced since the last flush (the flush waits for them)
_unpack_queued = -2         # id of the backward pass (autograd graph task) whose end-of-pass callback is queued
_rows_task = -2             # the pass the pending rows belong to


def _graph_task_id() -> int:
    """Id of the running backward pass (-1 outside one).  The end-of-pass callbacks are queued once per pass; keying the "queued"
    mark by the pass id (not a flag) means a pass that raised half-way cannot leave the mark set for every later pass."""
    f = getattr(torch._C, "_current_graph_task_id", None)
    return f() if f is not None else -1


def _begin_defer():
    """Rows left over from a pass that never reached its end (it raised): drop them and re-zero the workspaces they point to."""
    global _rows_task
    tid = _graph_task_id()
    if tid >= 0 and _rows_task != tid:
        if _unpack_rows or _gn_rows:
            reset_deferred_unpack()
        _rows_task = tid


def _queue_flush():
    global _unpack_queued
    tid = _graph_task_id()
    if tid < 0 or _unpack_queued != tid:       # (no id available: queue every time -- the flush is idempotent)
        _unpack_queued = tid
        torch.autograd.Variable._execution_engine.queue_callback(flush_deferred_unpack)


def _upload_table(rows, device):
    """int64 table -> device without stalling the host: a pageable source would make the copy wait for everything enqueued so far
    (the whole backward pass), once per new row set -- and the GroupNorm row sets (fresh allocations) take a few steps to repeat."""
    host = torch.tensor(rows, dtype=torch.int64)
    if device.type != "cuda":
        return host.to(device)
    host = host.pin_memory()
    if len(_pinned_tables) >= 4 * _TABLE_CACHE:
        del _pinned_tables[: 2 * _TABLE_CACHE]
    _pinned_tables.append(host)
    return host.to(device, non_blocking=True)


def _pending_table(pending, cache, table_row, device):
    """(device table, blocks) of a list of pending rows, from `cache` when this row set was flushed before (the workspaces are
    persistent, so the weight-gradient rows repeat from the second step on; the GroupNorm rows point into fresh allocations, whose
    addresses repeat only after a few steps).  table_row(row, begin) = the table's row for a pending row whose workgroups start at
    block `begin`: the exclusive prefix sum of the block counts, the last entry of every pending row."""
    global table_uploads
    key = tuple(pending)
    ent = cache.get(key)
    if ent is None:
        rows, begin = [], 0
        for r in pending:
            rows.append(table_row(r, begin))
            begin += r[-1]
        if len(cache) >= _TABLE_CACHE:
            cache.clear()
        ent = cache[key] = (_upload_table(rows, device), begin)
        table_uploads += 1
    return ent


def _note_producer_stream():
    if torch.cuda.is_available():
        st = torch.cuda.current_stream()
        _producer_streams[st.cuda_stream] = st


def _rest_workspace(weight, shape, like):
    key = (weight.data_ptr(), shape)
    ws = _rest_ws.get(key)
    if ws is None:
        ws = torch.zeros(shape, device=like.device, dtype=_f32)
        _rest_ws[key] = ws
    return ws


def _rest_workspace_for(weight, shape, like):
    """The layer's zero-at-rest workspace, flushed first when a row for it is already queued (a module applied twice in one
    forward pass: the second weight-gradient kernel may use plain stores, and two table rows with one workspace would be read,
    added and cleared from two block ranges -- ADVICE r2)."""
    ws = _rest_workspace(weight, shape, like)
    if ws.data_ptr() in _unpack_pending:
        flush_deferred_unpack()
    return ws


def _defer_unpack(ws, dst, co, ci, taps, cip, qkv):
    """Queue `dst (OIHW) += unpack(ws)` for the end-of-backward table launch; taps = 0 for the 2-D Winograd planes."""
    _begin_defer()
    items = co * ci * (taps if taps else 3)
    _unpack_rows.append((ws.data_ptr(), dst.data_ptr(), co, ci, taps, cip, int(qkv), 1, 1, (items + _UT_ITEMS - 1) // _UT_ITEMS))
    _unpack_keep.append((ws, dst))
    _unpack_pending.add(ws.data_ptr())
    _note_producer_stream()
    _queue_flush()


def _defer_gn_param(red, tot_off, ss, bstride, dgamma, dbeta, B, C):
    """Queue `dgamma, dbeta += batch reduction of the per-image sums` for the end-of-backward table launch."""
    _begin_defer()
    if dgamma.data_ptr() in _gn_pending:      # the same GroupNorm applied twice in one pass: its rows would race on dgamma / dbeta
        flush_deferred_unpack()
    _gn_rows.append((red.data_ptr() + 4 * tot_off, 0 if ss is None else ss.data_ptr(), int(bstride), dgamma.data_ptr(),
                     dbeta.data_ptr(), B, C, (C + 31) // 32))
    _gn_keep.append((red, ss, dgamma, dbeta))
    _gn_pending.add(dgamma.data_ptr())
    _note_producer_stream()
    _queue_flush()


def _used_on(stream, *tensors):
    """Tell the caching allocator that `tensors` are read by work enqueued on `stream`.  A block goes back to the pool of the
    stream it was ALLOCATED on as soon as its last reference drops; without this mark that stream could hand it out again and
    overwrite it while a kernel on `stream` is still reading (VERDICT r2 / ADVICE r2: the deferred GroupNorm rows are allocated
    by backward nodes on the main or the second-decoder stream and, with a bucketed reducer, flushed from inside a
    weight-gradient side-stream section).  A no-op for a tensor allocated on `stream` itself."""
    if stream is None:
        return
    for t in tensors:
        if t is not None and t.is_cuda:
            t.record_stream(stream)


def _flush_gn_params():
    if not _gn_rows:
        return
    table, blocks = _pending_table(_gn_rows, _gn_tables, lambda r, begin: list(r[:7]) + [begin], _gn_keep[0][0].device)
    call("adm_gn_bwd_param_table", ptr(table), len(_gn_rows), blocks)
    cur = torch.cuda.current_stream() if table.is_cuda else None
    _used_on(cur, table)            # (a cached table may have been uploaded on another stream and can be dropped by the cache)
    for red, ss, _dg, _db in _gn_keep:
        _used_on(cur, red, ss)      # fresh allocations of the GroupNorm backward nodes: released right below
    _gn_rows.clear()
    _gn_keep.clear()
    _gn_pending.clear()


def flush_deferred_unpack():
    """Scatter every pending weight-gradient workspace into its gradient (one launch) and clear the workspaces; reduce the pending
    GroupNorm parameter gradients (one launch)."""
    global _unpack_queued
    _unpack_queued = -2
    # whatever was queued must have landed: the weight gradients produced on the side stream (SIDE_WGRAD), the second decoder's
    # GroupNorm partial sums (BRANCH_STREAM), the main chain's when a reducer bucket flushes from inside a side-stream section
    if torch.cuda.is_available() and _producer_streams:
        cur = torch.cuda.current_stream()
        for key, st in list(_producer_streams.items()):
            if key != cur.cuda_stream:
                cur.wait_stream(st)
        _producer_streams.clear()
    _flush_gn_params()
    if not _unpack_rows:
        return
    table, blocks = _pending_table(_unpack_rows, _unpack_tables, lambda r, begin: list(r[:9]) + [begin, 0, 0], _unpack_keep[0][0].device)
    n = len(_unpack_rows)
    _unpack_rows.clear()         # (before the launch, unlike the GroupNorm rows: a launch that raises drops its rows)
    _unpack_keep.clear()         # (workspaces and gradient views are persistent: nothing is released here)
    _unpack_pending.clear()
    call("adm_unpack_wgrad_table", ptr(table), n, blocks)
    _used_on(torch.cuda.current_stream() if table.is_cuda else None, table)


def reset_deferred_unpack():
    """Drop pending rows and re-zero every workspace (after a backward pass that raised half-way)."""
    global _unpack_queued
    _unpack_queued = -2
    _unpack_rows.clear()
    _unpack_keep.clear()
    _unpack_pending.clear()
    _gn_rows.clear()
    _gn_keep.clear()
    _gn_pending.clear()
    for ws in _rest_ws.values():
        ws.zero_()


# ------------------------------------------------------------------------------------------------
# direct gradient accumulation
# ------------------------------------------------------------------------------------------------
# adm_amd.optim.FlatParams marks parameters whose .grad is a view into the flat gradient buffer
# (``p._adm_direct = True``).  For those, the backward kernels accumulate straight into ``p.grad``
# (saving a temporary, a zero-fill and autograd's ``grad += tmp`` pass per parameter) and return None
# to autograd; ``p._adm_grad_sink`` (set by the bucketed reducer) is then called in place of the
# post-accumulate-grad hook that autograd would have fired.
def _direct_grad(param):
    if param is not None and getattr(param, "_adm_direct", False) and param.grad is not None:
        return param.grad
    return None


def _mark_uses(ctx, *idx_params):
    """Forward side of _notify(): counts how often a directly-accumulated parameter takes part in the recorded graph, so that a
    module applied twice in one forward pass announces its gradient after the LAST of its backward nodes, as autograd's own
    accumulate-grad hook would (the bucketed reducer all-reduces a bucket as soon as every member has been announced)."""
    for i, p in idx_params:
        if p is not None and ctx.needs_input_grad[i] and getattr(p, "_adm_direct", False):
            p._adm_uses = getattr(p, "_adm_uses", 0) + 1


def _notify(param):
    # (a sink that READS the gradient -- the bucketed reducer when a bucket is complete -- calls flush_deferred_unpack() first:
    #  weight gradients and GroupNorm parameter gradients may still sit in their workspaces)
    uses = getattr(param, "_adm_uses", 0)
    if uses > 1:                       # more backward nodes of this parameter are still to come (FlatParams.zero_grad resets)
        param._adm_uses = uses - 1
        return
    param._adm_uses = 0
    sink = getattr(param, "_adm_grad_sink", None)
    if sink is not None:
        sink(param)


# Weight/bias gradients are side results of the backward chain: when they can be accumulated directly (flat gradient buffer) they
# are computed on a side stream, concurrently with the data-gradient chain on the main stream.  The split-bf16 kernels occupy a
# whole CU per workgroup, so the two streams never share a CU -- what overlaps is one kernel's tail (its last, partly filled round
# of workgroups and its slowest workgroups) with the next kernel's head.  Round 1 (f32-MFMA kernels at two workgroups per CU):
# 266.2 vs 265.2 ms/step, no gain, off.  Now (one workgroup per CU, ~350 us kernels): 149.6 vs 152.6 ms/step in the same run
# (855.6 vs 838.6 images/s) -- on by default with direct gradients; ADM_SIDE_WGRAD=0 keeps everything on one stream.
SIDE_WGRAD = os.environ.get("ADM_SIDE_WGRAD", "1") == "1"
_side_stream = None


def _wgrad_stream():
    global _side_stream
    if _side_stream is None:
        _side_stream = torch.cuda.Stream()
    return _side_stream


_join_queued = -2

# The two decoders of the two-output UNet are independent between the encoder and the preconditioning: the second one runs on its
# own stream (forward; autograd then runs its backward nodes there too), so that the kernels of the two chains fill each other's
# tails.  ADM_BRANCH_STREAM=0 keeps one stream.
BRANCH_STREAM = os.environ.get("ADM_BRANCH_STREAM", "1") == "1"
_branch_stream = None


def branch_stream():
    """The stream of the second decoder, made to wait for everything enqueued so far on the current stream; None when the branch
    must stay on the current stream (stream capture, switched off)."""
    global _branch_stream
    if not BRANCH_STREAM or not torch.cuda.is_available() or torch.cuda.is_current_stream_capturing():
        return None
    if _branch_stream is None:
        _branch_stream = torch.cuda.Stream()
    _branch_stream.wait_stream(torch.cuda.current_stream())
    return _branch_stream


def join_side_streams():
    global _join_queued
    _join_queued = -2
    if _side_stream is not None:
        torch.cuda.current_stream().wait_stream(_side_stream)
    if _branch_stream is not None:
        torch.cuda.current_stream().wait_stream(_branch_stream)


def _queue_join_at_end_of_backward():
    """Make the stream that called backward() wait for the side stream when the backward pass ends, so `.grad`
    is safe to read right after `loss.backward()` (same mechanism DDP uses for its final synchronisation)."""
    global _join_queued
    tid = _graph_task_id()
    if tid < 0 or _join_queued != tid:
        _join_queued = tid
        torch.autograd.Variable._execution_engine.queue_callback(join_side_streams)


# ------------------------------------------------------------------------------------------------
# convolution / linear
# ------------------------------------------------------------------------------------------------
def _use_wino(B, Ho, Wo, ks, up, tile) -> bool:
    """(Ho, Wo) = the grid the conv runs on; with `up` (fused nearest x2) both are even by construction."""
    return WINOGRAD and ks == 3 and tile < 0 and (Wo & 1) == 0 and _sel_batch(B) * Ho * Wo >= WINO_MIN_M


def _use_wino2d(B, Ho, Wo, ks, up, tile) -> bool:
    # the fused nearest-x2 layers take the 2-D form on the split-bf16 kernel only (conv_wino2d_x6.hip skips their zero pass)
    return WINOGRAD2D and (not up or BF16X6) and (Ho & 1) == 0 and _use_wino(B, Ho, Wo, ks, up, tile)


def _conv_data_pass(tag, x, x16, weight, pk, which, bias, res, y, ks, up, tile, qkv, bf16, amax, find_amax, *, gemm_m, gemm_ok,
                    h3_nosplit, bound_h3, bound_x6):
    """One stride-1 conv x -> y on the operands of direction `which` of a packed weight: 0 = the forward, 1 = the data gradient (the
    same conv over dy, cin and cout exchanged).  Selects the kernel and launches it; returns the bound vector that the kernel raised
    to max |y|, or None.  Where the two directions differ, the caller states the rule:
      amax / find_amax  the bound of x, or a function that looks it up -- called only where a fp16-format kernel could use the result
                        (under ADM_AMAX_CHECK the look-up reads the device)
      x16               the bf16-stored values of x (x is then only the f32 carrier), or None
      gemm_m            the pixel count that decides whether a 1x1 conv takes the split GEMM
      gemm_ok           False keeps a 1x1 conv off the split GEMM whatever its size
      h3_nosplit        batch_invariant() suppresses split-K on the fp16-format 3x3 kernel too (on every other kernel it always does)
      bound_h3 / _x6    the fp16-format / bf16-format 1x1 kernel leaves max |y|"""
    B, Ho, Wo, n_p = y.shape
    k_p = x.shape[-1]
    co, ci = weight.shape[0], weight.shape[1]
    use_bf16 = bf16 and k_p % 64 == 0
    if x16 is not None and not use_bf16:
        raise RuntimeError("a bf16-stored activation reached a conv that does not run in the bf16 mode")
    wino = not use_bf16 and _use_wino(B, Ho, Wo, ks, up, tile) and not qkv
    wino2 = wino and _use_wino2d(B, Ho, Wo, ks, up, tile)
    g6 = not use_bf16 and gemm_ok and _use_gemm_x6(gemm_m, ks, up, n_p, k_p)
    # fp16 format: the operand came with its max |x| ...
    if FP16X3 and ((wino2 and BF16X6) or (g6 and H3_GEMM)) and find_amax is not None:
        amax = find_amax(x)
    h3 = (wino2 and BF16X6 and FP16X3 and amax is not None
          and _h3_operands(weight, pk, which) is not None)           # ... and the weights fit their fp16 image
    wq2 = _wino2_operands(weight, pk, which) if (wino2 and not h3) else None
    wq = _wino_operands(weight, pk)[which] if (wino and not wino2) else None
    g6h = g6 and FP16X3 and H3_GEMM and amax is not None and _gemm_h3_operand(pk, which) is not None
    # small-M problems: split over the input channels into a workspace, fixed-order reduce
    sk = 1
    if _SELECT_BATCH is None or (h3 and not h3_nosplit):        # (not under batch_invariant(): the split count depends on the call's size)
        if wino2:
            sk = (hip.lib().adm_wino2d_x6_splitk if BF16X6 else hip.lib().adm_wino2d_splitk)(B, Ho, Wo, k_p, n_p)
        elif not (wino or g6 or use_bf16) and tile < 0:
            sk = hip.lib().adm_conv_splitk(B * Ho * Wo, n_p, ks * ks * k_p)
    ws = _new((sk * B * Ho * Wo * n_p,), x) if sk > 1 else None
    ws_n = 0 if ws is None else ws.numel()
    amax_y = None
    kind = ("wino2h3" if h3 else "wino2x6" if BF16X6 else "wino2") if wino2 else "wino" if wino else ("gemmh3" if g6h else "gemmx6") if g6 else "igemm"
    with _Prof(kind, 2.0 * B * Ho * Wo * co * ci * ks * ks,
               f"{tag}{'-' + kind if kind != 'igemm' else ''} M={B * Ho * Wo} N={n_p} K={ks * ks * k_p}"):
        if h3:
            # (no output bound from this kernel: tracking it in the epilogue cost the 96- / 128-cout forms ten more spilled registers,
            #  +10 % on their launches, for the handful of encoder skip convs that would have used it)
            call("adm_conv_fwd_wino2d_h3", ptr(x), ptr(_h3_operands(weight, pk, which)), ptr(bias), ptr(res), ptr(y), ptr(ws), ws_n,
                 B, Ho, Wo, k_p, k_p, n_p, n_p, n_p, n_p, _bptr(amax), H3_WSCALE, int(up))
        elif g6h:
            amax_y = _amax_slot(x) if bound_h3 else None
            call("adm_gemm_x6_h3", ptr(x), ptr(_gemm_h3_operand(pk, which)), ptr(bias), ptr(res), ptr(y), B * Ho * Wo, k_p, k_p, n_p,
                 n_p, n_p, n_p, _bptr(amax), H3_WSCALE, ptr(amax_y))
        elif g6 and bound_x6:
            amax_y = _amax_slot(x)
            call("adm_gemm_x6_amax", ptr(x), ptr(_gemm_x6_operand(pk, which)), ptr(bias), ptr(res), ptr(y), B * Ho * Wo, k_p, k_p, n_p,
                 n_p, n_p, n_p, ptr(amax_y))
        elif g6:
            call("adm_gemm_x6", ptr(x), ptr(_gemm_x6_operand(pk, which)), ptr(bias), ptr(res), ptr(y), B * Ho * Wo, k_p, k_p, n_p,
                 n_p, n_p, n_p)
        elif use_bf16:
            call("adm_conv_fwd_bf16a" if x16 is not None else "adm_conv_fwd_bf16", ptr(x16 if x16 is not None else x),
                 ptr(_bf16_operand(pk, "bwd" if which else "fwd")), ptr(bias), ptr(res), ptr(y), B, Ho, Wo, k_p, k_p, n_p, n_p, n_p,
                 n_p, ks, int(up), -1)
        elif wino2 and BF16X6:
            call("adm_conv_fwd_wino2d_x6_up" if up else "adm_conv_fwd_wino2d_x6", ptr(x), ptr(wq2), ptr(bias), ptr(res), ptr(y), ptr(ws),
                 ws_n, B, Ho, Wo, k_p, k_p, n_p, n_p, n_p, n_p)
        elif wino2:
            call("adm_conv_fwd_wino2d", ptr(x), ptr(wq2), ptr(bias), ptr(res), ptr(y), ptr(ws), ws_n, B, Ho, Wo, k_p, k_p, n_p, n_p,
                 n_p, n_p)
        elif wino:
            call("adm_conv_fwd_wino_up" if up else "adm_conv_fwd_wino", ptr(x), ptr(wq), ptr(bias), ptr(res), ptr(y), B, Ho, Wo,
                 k_p, k_p, n_p, n_p, n_p, n_p)
        elif sk > 1:
            call("adm_conv_fwd_ws", ptr(x), ptr(pk.bwd if which else pk.fwd), ptr(bias), ptr(res), ptr(y), ptr(ws), ws_n, B, Ho, Wo,
                 k_p, k_p, n_p, n_p, n_p, n_p, ks, int(up))
        else:
            call("adm_conv_fwd", ptr(x), ptr(pk.bwd if which else pk.fwd), ptr(bias), ptr(res), ptr(y), B, Ho, Wo, k_p, k_p, n_p,
                 n_p, n_p, n_p, ks, int(up), tile)
    return amax_y


def _wgrad_kind(B, Ho, Wo, ks, up, qkv, bf16, xdtype, bounds):
    """Which weight-gradient kernel a stride-1 conv takes, as the label the profiler gets, from the layer's facts and the module switches
    alone.  xdtype: how x is stored; bounds: both operands came with their max |.| (the fp16 format, conv_wgrad_x6.hip FMT 1).  Returns
    (kind, wmode, planes, conv_shaped): the packed tile's Winograd form, and whether the launch takes conv sizes or the GEMM's."""
    pow2 = lambda v: v > 0 and (v & (v - 1)) == 0
    wino_ok = _use_wino(B, Ho, Wo, ks, up, -1) and not qkv and pow2(Ho) and pow2(Wo)
    # bf16 mode with bf16 activation storage: the split-bf16 Winograd kernel (dy split exactly, x as stored) is faster than the
    # direct bf16 weight gradient (~250 vs 179 TFLOP/s algorithmic) and more accurate.  With f32 storage (ADM_BF16_STORAGE=0)
    # the direct kernel stays: it rounds x on load, so the two storage modes keep computing the same thing.
    xbf = xdtype == torch.bfloat16
    x6_bf = bf16 and xbf and BF16X6 and WINOGRAD2D and wino_ok and Ho >= 2
    wino = not bf16 and wino_ok
    wino2 = (wino and WINOGRAD2D and (not up or BF16X6) and Ho >= 2) or x6_bf   # 2-D F(3x3, 2x2): 12 x-folded planes per cout
    x6 = wino2 and BF16X6          # f32 products on the bf16 MFMA by exact three-term splitting (conv_wgrad_x6.hip)
    g6 = (GEMM_WGRAD_X6 and BF16X6 and (not bf16 or xbf) and ks == 1 and not up
          and B * Ho * Wo >= GEMM_X6_MIN_M)      # ... 1x1 convs (its MODE 1)
    h3 = bounds and (x6 or g6) and not bf16 and H3_WGRAD
    kind = "wgrad_wino2h3" if (h3 and x6) else "wgrad_gemmh3" if h3 else "wgrad_wino2x6" if x6 else "wgrad_gemmx6" if g6 else "wgrad_wino2" if wino2 else "wgrad_wino" if wino else "wgrad"
    return kind, 2 if wino2 else int(wino), 12 if wino2 else ks * ks, not kind.startswith("wgrad_gemm")


def _wgrad_workspace(kind, det, defer, weight, like, B, Ho, Wo, cip, cop, ks, up, wmode, planes, need_b):
    """(dwp, splits, bws): what a weight-gradient kernel of `kind` writes.  det: `splits` partial tiles by the kernel's own plan query
    and, with need_b, as many bias rows bws; defer: the layer's zero-at-rest workspace, which the end-of-backward table unpacks and
    clears; else a fresh tile.  splits = 0 and bws = None outside det."""
    if det:        # splits store partial tiles to a workspace; the unpack launch sums them in a fixed order
        splits = (hip.lib().adm_conv_wgrad_x6_plan(B, Ho, Wo, cip, cop) if kind in ("wgrad_wino2x6", "wgrad_wino2h3") else
                  hip.lib().adm_gemm_wgrad_x6_plan(B * Ho * Wo, cip, cop) if kind.startswith("wgrad_gemm") else
                  hip.lib().adm_conv_wgrad_plan(B, Ho, Wo, cip, cop, ks, int(up), wmode))
        if splits < 1:
            raise RuntimeError(f"adm_conv_wgrad_plan failed with code {splits}")
        return _new((splits, cop, planes * cip), like), splits, (_new((splits, cop), like) if need_b else None)
    if defer:
        _begin_defer()          # (before the kernel: a pass that died may have left this workspace dirty)
        return _rest_workspace_for(weight, (cop, planes * cip), like), 0, None
    return _new((cop, planes * cip), like), 0, None


def _unpack_wgrad(weight, sink, dwp, ks, qkv, wino2, defer, splits, bws, dbk):
    """The packed tile dwp -> the OIHW gradient: added into `sink` (the flat gradient buffer's view; the caller then announces it with
    _notify, after what it still has to finish) or stored to a new tensor, which is returned for autograd.  defer: as a row of the
    end-of-backward table; splits > 0: sums that many partial tiles, and the bias rows bws into dbk; wino2: 2-D Winograd planes."""
    co, ci = weight.shape[0], weight.shape[1]
    cop, cip = ceil32(co), ceil32(ci)
    dst = sink if sink is not None else _like(weight)
    acc = int(sink is not None)
    if defer:
        _defer_unpack(dwp, dst, co, ci, 0 if wino2 else ks * ks, cip, qkv)
    elif wino2:    # the y half of G^T rides in the unpack: dW[ky] = sum_ey Gt[ky][ey] wx[ey]
        call("adm_unpack_wgrad_wino2d", ptr(dwp), splits or 1, ptr(dst), co, ci, cop, cip, acc, ptr(bws) if splits else None,
             ptr(dbk) if splits else None)
    elif splits:
        call("adm_unpack_wgrad_splits", ptr(dwp), splits, ptr(dst), co, ci, ks, cop, cip, int(qkv), acc, ptr(bws), ptr(dbk))
    else:
        call("adm_unpack_wgrad", ptr(dwp), ptr(dst), co, ci, ks, cop, cip, int(qkv), acc)
    return None if sink is not None else dst


def _finish_bias(bias_to, dbp, bsink, bias, co, qkv, dy):
    """The bias gradient from where the kernels left it (dbp, packed order) to where the route `bias_to` of _Conv.backward sends it;
    returns db for autograd, None when the flat gradient buffer took it (then announced here)."""
    db = dbp if bias_to == "fresh" else None
    if bias_to == "table":
        _defer_unpack(dbp, bsink, co, 1, 1, 1, qkv)
    elif bias_to == "permute":
        db = _new((co,), dy)
        call("adm_permute_vec", ptr(dbp), ptr(db), co, co, int(qkv), 1)
    if bias_to in ("sink", "table"):
        _notify(bias)
    return db


def _conv_param_pass(x, dy, weight, bias, ks, up, qkv, bf16, amax_x, need_w, wsink, bias_to, bsink):
    """The weight and bias gradients of a stride-1 conv from its saved input x and dy: selects the weight-gradient kernel and its
    workspace, launches, unpacks and hands over.  Returns (dw, db) for autograd, None where the flat gradient buffer took one or none
    was asked for.  The caller states:
      amax_x          the bound x came with on the fp16 format, or None (dy's is looked up only where it would change the kernel)
      need_w, wsink   the weight needs a gradient; its view of the flat gradient buffer, or None
      bias_to, bsink  the bias gradient's route (None: not needed); its view of the flat gradient buffer, or None"""
    B, Ho, Wo, cop = dy.shape
    co, ci = weight.shape[0], weight.shape[1]
    cip = ceil32(ci)
    # fp32: the weight-gradient kernel also produces the bias gradient (column sums of dy) on its way
    fused_b = bias_to is not None and need_w and not bf16
    # dbp: where the kernel (fused_b: it accumulates) or adm_colsum (it stores) leaves the bias gradient, in packed order
    dbp = None
    if bias_to == "sink":
        dbp = bsink
    elif bias_to == "table":
        _begin_defer()
        dbp = _rest_workspace_for(bias, (cop,), dy)
    elif bias_to is not None:
        n = co if bias_to == "fresh" else cop
        dbp = torch.zeros((n,), device=dy.device, dtype=_f32) if fused_b else _new((n,), dy)
    dw = db = None
    if need_w:
        dbk = dbp if fused_b else None      # (what the kernel is given)
        det = DETERMINISTIC and not bf16
        defer = DEFER_UNPACK and wsink is not None and not det      # (with a side stream: the flush joins it first)
        facts = (B, Ho, Wo, ks, up, qkv, bf16, x.dtype)
        kind, wmode, planes, conv_shaped = _wgrad_kind(*facts, False)
        dwp, splits, bws = _wgrad_workspace(kind, det, defer, weight, dy, B, Ho, Wo, cip, cop, ks, up, wmode, planes, fused_b)
        # fp16 format (conv_wgrad_x6.hip FMT 1): both operands came with their bounds
        kind_h3 = _wgrad_kind(*facts, True)[0]
        amax_dy = _get_amax(dy) if amax_x is not None and kind_h3 != kind else None
        if amax_dy is not None:
            _check_bound(x, amax_x, "a conv input (weight gradient)")
            kind = kind_h3
        # x, dy, the packed dW tile and the bias gradient's rows (per split under det); then conv-shaped or GEMM-shaped sizes
        head = (ptr(x), ptr(dy), ptr(dwp), ptr(bws if det else dbk))
        size = (B, Ho, Wo, cip, cip, cop, cop) if conv_shaped else (B * Ho * Wo, cip, cip, cop, cop)
        nsplit = splits if det else -1 if defer else 0       # -1: chosen by the launcher, workspace zero on entry (no memset)
        with _Prof(kind, 2.0 * B * Ho * Wo * co * ci * ks * ks,
                   f"{kind.replace('_', '-')} P={B * Ho * Wo} Co={cop} Ci={cip} ks={ks}"):
            if kind == "wgrad_wino2h3":
                call("adm_conv_wgrad_x6_h3", *head, *size, nsplit, int(up), int(det), _bptr(amax_x), _bptr(amax_dy))
            elif kind == "wgrad_gemmh3":
                call("adm_gemm_wgrad_x6_h3", *head, *size, nsplit, int(det), _bptr(amax_x), _bptr(amax_dy))
            elif kind == "wgrad_gemmx6":
                call("adm_gemm_wgrad_x6_bf16a" if bf16 else "adm_gemm_wgrad_x6_ws" if det else "adm_gemm_wgrad_x6", *head, *size, nsplit)
            elif kind == "wgrad_wino2x6" and (bf16 or det):
                call("adm_conv_wgrad_x6_bf16a" if bf16 else "adm_conv_wgrad_x6_ws", *head, *size, nsplit, int(up))
            elif kind == "wgrad_wino2x6":
                call("adm_conv_wgrad_x6_up" if up else "adm_conv_wgrad_x6", *head, *size, nsplit)
            elif bf16:       # (no bias gradient from the direct bf16 kernels)
                call("adm_conv_wgrad_bf16a" if x.dtype == torch.bfloat16 else "adm_conv_wgrad_bf16", *head[:3], *size, ks, int(up), nsplit)
            elif det:
                call("adm_conv_wgrad_ws", *head, *size, ks, int(up), nsplit, wmode)
            elif kind == "wgrad_wino2":
                call("adm_conv_wgrad_wino2d", *head, *size, nsplit)
            elif kind == "wgrad_wino":
                call("adm_conv_wgrad_wino_up" if up else "adm_conv_wgrad_wino", *head, *size, nsplit)
            else:
                call("adm_conv_wgrad_bias", *head, *size, ks, int(up), nsplit)
        dw = _unpack_wgrad(weight, wsink, dwp, ks, qkv, wmode == 2, defer, splits, bws, dbk)
        if fused_b:
            db = _finish_bias(bias_to, dbp, bsink, bias, co, qkv, dy)
        if wsink is not None:
            _notify(weight)
    if bias_to is not None and not fused_b:
        call("adm_colsum", ptr(dy), ptr(dbp), B * Ho * Wo, cop, cop, int(bias_to == "sink"))
        db = _finish_bias(bias_to, dbp, bsink, bias, co, qkv, dy)
    return dw, db


class _Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, ks, up, qkv, tile, amax=None):
        x = _chk(x, "x")
        B, H, W, cx = x.shape
        co, ci = weight.shape[0], weight.shape[1]
        cop, cip = ceil32(co), ceil32(ci)
        if cx != cip:
            raise RuntimeError(f"conv input has {cx} channels, expected {cip} (= ceil32({ci}))")
        pk = packed(weight, bias, ks, qkv)
        Ho, Wo = (2 * H, 2 * W) if up else (H, W)
        y = _new((B, Ho, Wo, cop), x)
        res = None
        if residual is not None:
            res = _chk(residual, "residual")
            if tuple(res.shape) != tuple(y.shape):
                raise RuntimeError(f"residual shape {tuple(res.shape)} != output {tuple(y.shape)}")
        bf16 = COMPUTE == "bf16"
        x16 = getattr(x, "_adm_bf16", None)          # bf16-storage mode: the values of this input live here (x is the f32 carrier)
        # the bound of a 1x1 conv's OUTPUT (qkv -> attention -> proj; proj + residual -> the next block's skip conv): written by the epilogue
        # (bias and residual included) and handed to the consumer on y, where conv2d / attention look for it
        fmt = _fp16_format()
        want_out = fmt and H3_GEMM
        amax_y = _conv_data_pass("fwd", x, x16, weight, pk, 0, pk.bias, res, y, ks, up, tile, qkv, bf16, amax, None,
                                 gemm_m=_sel_batch(B) * Ho * Wo, gemm_ok=True, h3_nosplit=True, bound_h3=want_out, bound_x6=want_out)
        ctx.save_for_backward(x16 if x16 is not None else x, weight, bias)      # (the carrier is not kept)
        _mark_uses(ctx, (1, weight), (2, bias))
        ctx.meta = (ks, up, qkv, residual is not None, bf16)
        ctx.amax_x = amax if fmt else None       # the weight gradient reads x on the same format
        if amax_y is not None:
            y._adm_amax = amax_y
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias = ctx.saved_tensors
        ks, up, qkv, has_res, bf16 = ctx.meta
        dy = _chk(dy, "dy")
        B, Ho, Wo, cop = dy.shape
        co, ci = weight.shape[0], weight.shape[1]
        cip = ceil32(ci)
        dx = dw = db = None
        need_w = ctx.needs_input_grad[1]
        wsink = _direct_grad(weight) if need_w else None
        bsink = _direct_grad(bias) if ctx.needs_input_grad[2] else None
        # how the bias gradient travels -- the one place that decides it
        bias_to = None
        if bias is not None and ctx.needs_input_grad[2]:
            if not qkv and cop == co:       # the packed order is the parameter's:
                bias_to = "sink" if bsink is not None else "fresh"      # straight into the flat gradient buffer / a new [co] for autograd
            # a bias whose packed order differs from its parameter's (qkv interleave, padded couts) goes through a zero-at-rest vector and a
            # row of the end-of-backward table (which permutes, accumulates and clears) instead of zeros + permute + autograd's add
            elif bsink is not None and not bf16 and DEFER_UNPACK and not DETERMINISTIC and wsink is not None:
                bias_to = "table"
            else:
                bias_to = "permute"         # a padded temporary, then adm_permute_vec into a new [co] for autograd
        params = (x, dy, weight, bias, ks, up, qkv, bf16, ctx.amax_x, need_w, wsink, bias_to, bsink)
        side = None
        if SIDE_WGRAD and PROFILE is None and wsink is not None and bias_to in (None, "sink", "table"):    # (nothing goes back through autograd)
            side = _wgrad_stream()
            ev = torch.cuda.Event()
            ev.record()                      # dy (and x) are complete at this point of the main stream
            side.wait_event(ev)
            _queue_join_at_end_of_backward()
            with torch.cuda.stream(side):
                dw, db = _conv_param_pass(*params)
            dy.record_stream(side)           # keep the allocator from recycling them under the side stream
            x.record_stream(side)
        if ctx.needs_input_grad[0]:
            pk = packed(weight, bias, ks, qkv)
            dxf = _new((B, Ho, Wo, cip), dy)
            # gemm_ok: a data gradient that sums fewer than 32 real couts stays on the f32 kernel: over so few terms the split formats'
            #  truncated cross products are not averaged out, and a head's dx over 1 or 3 couts measured 1.05-1.39x of twice the f32
            #  kernel's rms error against fp64, tests/test_hip_accuracy.py
            #  (and no fused nearest-x2 1x1 conv ever took the split GEMM here)
            # bound_h3: the epilogue leaves max |dx| (the attention backward behind a proj conv runs on the fp16 format); there is no
            #  adm_gemm_x6_amax on this side
            slot_dx = _conv_data_pass("dgrad", dy, None, weight, pk, 1, None, None, dxf, ks, False, -1, qkv, bf16, None, _get_amax,
                                      gemm_m=B * Ho * Wo, gemm_ok=co >= 32 and not up, h3_nosplit=False, bound_h3=True, bound_x6=False)
            if slot_dx is not None:
                _reg_amax(dxf, slot_dx)
            if up:   # gradient of nearest x2 = 2x2 sum
                dx = _new((B, Ho // 2, Wo // 2, cip), dy)
                call("adm_resample2x", ptr(dxf), ptr(dx), B, Ho, Wo, cip, 0, 1.0, 0)
            else:
                dx = dxf
        if side is None:             # one stream: after the data gradient
            dw, db = _conv_param_pass(*params)
        return dx, dw, db, (dy if has_res else None), None, None, None, None, None


def conv2d(x, weight, bias=None, residual=None, *, up=False, qkv=False, tile=-1, amax=None):
    """NHWC conv: weight OIHW with k in {1,3}; optional fused nearest-x2 (``up``) and residual add.  amax: a device float >= max |x|
    (default: the one a GroupNorm kernel attached to x) -- lets the 3x3 layers run on the fp16 split format."""
    if amax is None:
        amax = getattr(x, "_adm_amax", None)
    _check_bound(x, amax, "a conv input")
    return _Conv.apply(x, weight, bias, residual, weight.shape[-1] if weight.dim() == 4 else 1, bool(up), bool(qkv), tile, amax)


def linear(x, weight, bias=None, residual=None):
    """x [B, in_pad] @ weight[out, in].T + bias (+ residual): the same implicit-GEMM kernel with H=W=1."""
    B = x.shape[0]
    r = None if residual is None else residual.reshape(B, 1, 1, -1)
    y = _Conv.apply(x.reshape(B, 1, 1, -1), weight, bias, r, 1, False, False, -1)
    return y.reshape(B, -1)


# ------------------------------------------------------------------------------------------------
# GroupNorm + scale/shift + SiLU + dropout
# ------------------------------------------------------------------------------------------------
_drop_counter = itertools.count(1)


def next_dropout_seed() -> int:
    return (torch.initial_seed() * 0x9E3779B1 + next(_drop_counter) * 0x85EBCA6B) & 0xFFFFFFFFFFFFFFFF


class _GroupNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, ss, silu, drop_p, seed, groups=0, eps=1e-5, fork=False, out_bf16=False, slot=None, slot_flag=None,
                want_amax=False):
        x_in = x
        x = _chk(x, "x")
        B, H, W, C = x.shape
        G = groups if groups else min(32, C // 4)
        HW = H * W
        g, b = _chk(gamma.detach(), "gamma"), _chk(beta.detach(), "beta")
        S = hip.lib().adm_gn_splits(HW, C)
        stats = _new((B, G, 2), x)
        ws = _new((B * S * G * 2,), x, torch.float64)
        prof = _Prof("gn", 8.0 * x.numel(), f"gn-fwd B={B} HW={HW} C={C} drop={int(drop_p > 0)} (TB/s)")
        prof.__enter__()
        ssc, bstride = None, 0
        if ss is not None:           # (slot, slot_flag: affine_group()'s slice of the one dss buffer for this block + its "written" mark)
            if ss.dim() == 2 and ss.stride(1) == 1 and ss.stride(0) >= ss.shape[1] and ss.dtype == _f32 and ss.is_cuda:
                ssc = ss                                  # a column slice of a wide [B, sum 2C] buffer is read in place (row stride)
            else:
                ssc = _chk(ss, "scale_shift")
            if ssc.shape[-1] != 2 * C or ssc.shape[0] not in (1, B):
                raise RuntimeError(f"scale/shift shape {tuple(ssc.shape)} does not match C={C}, B={B}")
            bstride = 0 if ssc.shape[0] == 1 else (ssc.stride(0) if ssc.dim() == 2 else 2 * C)
        y = _like(x)
        if out_bf16 and C % 64 == 0:
            # bf16 storage: the VALUES go to y16; `y` is only the f32 shape / dtype carrier autograd needs between this node and the
            # conv that consumes it (its storage is never written or read, and is released as soon as the conv has run)
            y16 = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
            call("adm_gn_fwd_bf16out", ptr(x), ptr(stats), ptr(ws), ptr(g), ptr(b), ptr(ssc), bstride, ptr(y16), B, HW, C, G, float(eps),
                 int(silu), float(drop_p), seed)
            y._adm_bf16 = y16       # conv2d looks for the values here
        else:
            if want_amax:     # the conv that consumes y runs on the fp16 format: it needs max |y| (written next to y by the same kernel)
                slot_a = _amax_slot(x)
                call("adm_gn_fwd_amax", ptr(x), ptr(stats), ptr(ws), ptr(g), ptr(b), ptr(ssc), bstride, ptr(y), ptr(slot_a), B, HW, C, G,
                     float(eps), int(silu), float(drop_p), seed)
                y._adm_amax = slot_a      # conv2d looks for the bound on its input
            else:
                call("adm_gn_fwd", ptr(x), ptr(stats), ptr(ws), ptr(g), ptr(b), ptr(ssc), bstride, ptr(y), B, HW, C, G, float(eps),
                     int(silu), float(drop_p), seed)
        prof.__exit__()
        ctx.save_for_backward(x, gamma, beta, ssc, stats)
        ctx.meta = (G, S, bstride, silu, drop_p, seed)
        ctx.slot, ctx.slot_flag = (slot, slot_flag) if ss is not None else (None, None)
        _mark_uses(ctx, (1, gamma), (2, beta))
        if fork:          # second output = the input itself, for the residual branch; its gradient comes back as `dxr`
            return y, x_in
        return y

    @staticmethod
    def backward(ctx, dy, dxr=None):
        x, gamma, beta, ss, stats = ctx.saved_tensors
        G, S, bstride, silu, drop_p, seed = ctx.meta
        if dy is None:    # only the pass-through output was used
            return dxr, None, None, None, None, None, None, None, None, None, None, None, None, None
        dy = _chk(dy, "dy")
        add = None if dxr is None else _chk(dxr, "residual gradient")
        B, H, W, C = x.shape
        HW = H * W
        dx = _like(x)
        dss = None
        slot = ctx.slot
        if ss is not None and ctx.needs_input_grad[3]:
            if bstride == 0 and B > 1:
                raise RuntimeError("backward through a batch-broadcast scale/shift is not supported")
            if slot is not None and bstride == slot.stride(0):
                dss = slot               # written in place into the group's [B, sum 2C] gradient buffer (same row stride as ss)
            else:
                slot = None
                if bstride not in (0, 2 * C):
                    raise RuntimeError("a strided scale/shift needs its gradient slot (ops.affine_group)")
                dss = _new((B, 2 * C), x)
        sg, sb = _direct_grad(gamma), _direct_grad(beta)
        direct = sg is not None and sb is not None
        dgamma = sg if direct else torch.zeros_like(gamma)
        dbeta = sb if direct else torch.zeros_like(beta)
        red = _new((B * S * C * 2 + B * C * 2 + B * G * 2,), x)
        defer = direct and DEFER_UNPACK and not DETERMINISTIC      # the batch reduction joins the end-of-backward table launch
        if defer:
            _begin_defer()
        slot_a = _amax_slot(x) if _fp16_format() else None      # max |dx| for the conv that consumes dx
        with _Prof("gn", (12.0 if add is None else 16.0) * x.numel(), f"gn-bwd B={B} HW={HW} C={C} drop={int(drop_p > 0)} (TB/s)"):
            if slot_a is not None:
                call("adm_gn_bwd_add_amax", ptr(x), ptr(dy), ptr(stats), ptr(gamma.detach()), ptr(beta.detach()), ptr(ss), bstride,
                     ptr(add), ptr(dx), ptr(dss), None if defer else ptr(dgamma), None if defer else ptr(dbeta), ptr(red), ptr(slot_a),
                     B, HW, C, G, int(silu), float(drop_p), seed)
            else:
                call("adm_gn_bwd_add", ptr(x), ptr(dy), ptr(stats), ptr(gamma.detach()), ptr(beta.detach()), ptr(ss), bstride,
                     ptr(add), ptr(dx), ptr(dss), None if defer else ptr(dgamma), None if defer else ptr(dbeta), ptr(red), B, HW, C, G,
                     int(silu), float(drop_p), seed)
        _reg_amax(dx, slot_a)
        if defer:
            _defer_gn_param(red, B * S * C * 2, ss, bstride, dgamma, dbeta, B, C)
        if slot is not None:
            ctx.slot_flag[0] = True
            dss = None                   # (the group's backward node reads the buffer; autograd carries nothing for this edge)
        if direct:
            _notify(gamma); _notify(beta)
            return dx, None, None, dss, None, None, None, None, None, None, None, None, None, None
        return dx, dgamma, dbeta, dss, None, None, None, None, None, None, None, None, None, None


def _want_amax(to_conv) -> bool:
    return bool(to_conv) and _fp16_format()


def group_norm_act(x, gamma, beta, scale_shift=None, *, silu=True, drop_p=0.0, seed=0, groups=0, eps=1e-5, to_conv=False, bound=False):
    """groups = 0: the UNet's min(32, C // 4) (uncond_unet.py:119-129); the KL autoencoder passes 32 / 1e-6
    (ddm/encoder_decoder.py:56-57).  to_conv=True promises that the ONLY consumer of the result is ops.conv2d: in the bf16-storage
    mode the values are then written as bf16 and the returned f32 tensor is an unwritten carrier (see _GroupNormAct.forward)."""
    out16 = bool(to_conv) and bf16_storage()
    slot = getattr(scale_shift, "_adm_dss", None) if scale_shift is not None else None       # (set by affine_group())
    wa = _want_amax(to_conv or bound)         # bound=True: the consumer is a conv behind a 2x2 mean (which keeps the bound)
    return _GroupNormAct.apply(x, gamma, beta, scale_shift, bool(silu), float(drop_p), int(seed), int(groups), float(eps), False, out16,
                               None if slot is None else slot[0], None if slot is None else slot[1], wa)


def group_norm_act_fork(x, gamma, beta, scale_shift=None, *, silu=True, drop_p=0.0, seed=0, groups=0, eps=1e-5, to_conv=False, bound=False):
    """(group_norm_act(x), x): the second output is x itself, to be used by the residual branch of a block.  In backward
    the residual branch's gradient arrives together with the normalised branch's, and is added inside the GroupNorm
    backward kernel instead of by a separate autograd accumulation pass (4 instead of 12 bytes per element)."""
    if not (torch.is_grad_enabled() and x.requires_grad):
        return group_norm_act(x, gamma, beta, scale_shift, silu=silu, drop_p=drop_p, seed=seed, groups=groups, eps=eps, to_conv=to_conv,
                              bound=bound), x
    out16 = bool(to_conv) and bf16_storage()
    wa = _want_amax(to_conv or bound)
    y, xo = _GroupNormAct.apply(x, gamma, beta, scale_shift, bool(silu), float(drop_p), int(seed), int(groups), float(eps), True, out16,
                                None, None, wa)
    a = getattr(x, "_adm_amax", None)
    if a is not None:
        xo._adm_amax = a             # (xo is x: the skip / residual branch keeps its bound; an input that is returned does not keep attributes)
    return y, xo


# A decoder block's input is z = cat(x, scale * skip), and the first thing the block does is norm0.fork(z).  The GroupNorm kernels sit
# on both sides of that copy with one thread per channel quad, so they pick a source (forward) or destination (backward) per thread:
# adm_gn_fwd_cat_amax reads the two halves in its moments pass and writes z (the 1x1 skip conv and its weight gradient still read it) as
# a side output, adm_gn_bwd_add_cat_amax writes the two gradient halves in place of dz.  Against concat_channels + group_norm_act_fork
# that is one read of z less forward, one write and one read of dz less backward, and two launches less; the results are bit-identical.
# ADM_GN_CONCAT=0 keeps the two-step path.
GN_CONCAT = os.environ.get("ADM_GN_CONCAT", "1") != "0"


class _GroupNormActCat(torch.autograd.Function):
    """(a, b) -> (act(norm(z)), z) with z = cat(a, scale_b * b): _Concat + _GroupNormAct(fork=True) without the copy passes."""

    @staticmethod
    def forward(ctx, a, b, scale_b, gamma, beta, silu, groups, eps, want_amax):
        a, b = _chk(a, "a"), _chk(b, "b")
        B, H, W, ca = a.shape
        cb = b.shape[-1]
        C, HW = ca + cb, H * W
        G = groups if groups else min(32, C // 4)
        g, bt = _chk(gamma.detach(), "gamma"), _chk(beta.detach(), "beta")
        S = hip.lib().adm_gn_splits(HW, C)
        z = _new((B, H, W, C), a)
        y = _like(z)
        stats = _new((B, G, 2), a)
        ws = _new((B * S * G * 2,), a, torch.float64)
        slot_z = _amax_slot(a) if (_fp16_format() and H3_GEMM) else None      # as _Concat: the 1x1 skip conv reads z
        slot_y = _amax_slot(a) if want_amax else None                        # as _GroupNormAct: conv0 reads y
        # (the `gn` record keeps its minimal-bytes convention, one read and one write of the map: the z store is not counted)
        with _Prof("gn", 8.0 * z.numel(), f"gn-fwd-cat B={B} HW={HW} C={ca}+{cb} drop=0 (TB/s)"):
            call("adm_gn_fwd_cat_amax", ptr(a), ca, ptr(b), cb, float(scale_b), ptr(z), ptr(slot_z), ptr(stats), ptr(ws), ptr(g), ptr(bt),
                 None, 0, ptr(y), ptr(slot_y), B, HW, G, float(eps), int(silu), 0.0, 0)
        if slot_z is not None:
            z._adm_amax = slot_z
        if slot_y is not None:
            y._adm_amax = slot_y
        ctx.save_for_backward(z, gamma, beta, stats)
        ctx.meta = (G, S, silu, ca, cb, scale_b)
        _mark_uses(ctx, (3, gamma), (4, beta))
        return y, z

    @staticmethod
    def backward(ctx, dy, dz):
        z, gamma, beta, stats = ctx.saved_tensors
        G, S, silu, ca, cb, scale_b = ctx.meta
        B, H, W, C = z.shape
        HW = H * W
        da, db = _new((B, H, W, ca), z), _new((B, H, W, cb), z)
        if dy is None:    # only z was used: what is left is _Concat.backward
            dz = _chk(dz, "dz")
            call("adm_split2", ptr(dz), ptr(da), ca, ptr(db), cb, B * HW, float(scale_b))
            bound = _get_amax(dz)
            if bound is not None:
                _reg_amax(da, bound)
                if abs(scale_b) <= 1.0:
                    _reg_amax(db, bound)
            return da, db, None, None, None, None, None, None, None
        dy = _chk(dy, "dy")
        add = None if dz is None else _chk(dz, "residual gradient")
        sg, sb = _direct_grad(gamma), _direct_grad(beta)
        direct = sg is not None and sb is not None
        dgamma = sg if direct else torch.zeros_like(gamma)
        dbeta = sb if direct else torch.zeros_like(beta)
        red = _new((B * S * C * 2 + B * C * 2 + B * G * 2,), z)
        defer = direct and DEFER_UNPACK and not DETERMINISTIC      # the batch reduction joins the end-of-backward table launch
        if defer:
            _begin_defer()
        slot_a = _amax_slot(z) if _fp16_format() else None      # max |dz|: bounds da, and db where |scale_b| <= 1 (as _Concat.backward)
        with _Prof("gn", (12.0 if add is None else 16.0) * z.numel(), f"gn-bwd-cat B={B} HW={HW} C={ca}+{cb} drop=0 (TB/s)"):
            call("adm_gn_bwd_add_cat_amax", ptr(z), ptr(dy), ptr(stats), ptr(gamma.detach()), ptr(beta.detach()), None, 0, ptr(add),
                 ptr(da), ca, ptr(db), cb, float(scale_b), None, None if defer else ptr(dgamma), None if defer else ptr(dbeta), ptr(red),
                 ptr(slot_a), B, HW, G, int(silu), 0.0, 0)
        _reg_amax(da, slot_a)
        if abs(scale_b) <= 1.0:
            _reg_amax(db, slot_a)
        if defer:
            _defer_gn_param(red, B * S * C * 2, None, 0, dgamma, dbeta, B, C)
        if direct:
            _notify(gamma); _notify(beta)
            return da, db, None, None, None, None, None, None, None
        return da, db, None, dgamma, dbeta, None, None, None, None


def _gn_cat_ok(a, b, groups) -> bool:
    """The fused concat form applies: f32 NHWC tensors on the GPU, whole channel quads on both sides, a shape the GroupNorm kernels take."""
    if not (GN_CONCAT and a.is_cuda and b.is_cuda and a.dim() == 4 and a.shape[:-1] == b.shape[:-1] and a.dtype == _f32 and b.dtype == _f32):
        return False
    if bf16_storage():
        return False
    ca, cb = a.shape[-1], b.shape[-1]
    C = ca + cb
    if ca <= 0 or cb <= 0 or ca % 4 or cb % 4:
        return False
    plan = (ctypes.c_int * 5)()
    return hip.lib().adm_gn_plan(a.shape[1] * a.shape[2], C, groups if groups else min(32, C // 4), plan) == 0


def group_norm_act_cat(a, b, scale_b, gamma, beta, *, silu=True, groups=0, eps=1e-5, to_conv=False, bound=False):
    """(group_norm_act(z), z) for z = cat(a, scale_b * b) along the channels: concat_channels + group_norm_act_fork as one op (see
    GN_CONCAT above); the two-step path where the fused kernels do not apply."""
    if not _gn_cat_ok(a, b, groups):
        z = concat_channels(a, b, scale_b)
        return group_norm_act_fork(z, gamma, beta, None, silu=silu, groups=groups, eps=eps, to_conv=to_conv, bound=bound)
    return _GroupNormActCat.apply(a, b, float(scale_b), gamma, beta, bool(silu), int(groups), float(eps), _want_amax(to_conv or bound))


# ------------------------------------------------------------------------------------------------
# all `affine` Linears of a UNet as ONE GEMM (and their gradients as two)
# ------------------------------------------------------------------------------------------------
# Every UNetBlock maps the same embedding [B, E] through its own Linear(E, 2 C) to the scale / shift of its second GroupNorm
# (uncond_unet.py:167, 195-196): 57 launches of ~16 us on 128 rows forward, 57 + 57 backward plus 56 autograd additions of the
# embedding gradient.  The packed forward operands [2C][E] of the blocks are rows of one [sum 2C][E] matrix if they sit next to
# each other in memory -- so they are re-homed into one buffer (the per-step repack table writes them there), the scale/shift of ALL
# blocks is one GEMM, every block reads ITS columns in place (row stride = sum 2C, adm_gn_fwd's ss_bstride), the GroupNorm backward
# writes d scale/shift into the same columns of one gradient buffer, and the Linears' backward is one data-gradient GEMM
# (K = sum 2C, split over K) and one weight-gradient launch whose tile rows go to the blocks' gradients through the deferred unpack
# table.  ADM_AFFINE_GROUP=0 keeps the per-block Linears.
AFFINE_GROUP = os.environ.get("ADM_AFFINE_GROUP", "1") != "0"


class AffineGroup:
    """Host-side state of the grouped Linears: layer list, column offsets, the re-homed operand buffers."""

    def __init__(self, linears):
        self.linears = list(linears)
        w0 = self.linears[0].weight
        self.K = w0.shape[1]
        if self.K % 32 or any(l.weight.shape[1] != self.K or l.weight.shape[0] % 32 or l.bias is None for l in self.linears):
            raise RuntimeError("affine_group: every Linear must map the same, 32-aligned embedding width to a 32-aligned width, with a bias")
        self.widths = [l.weight.shape[0] for l in self.linears]
        self.offsets = [0]
        for n in self.widths:
            self.offsets.append(self.offsets[-1] + n)
        self.total = self.offsets[-1]
        self.wcat = self.wcat_t = self.bcat = self.t_table = None
        self.sig = self.sig_t = None
        self.bias_table = None
        self.ws_w = self.ws_b = None          # zero-at-rest weight / bias gradient tiles (deferred unpack)

    def operands(self):
        """Current [total][K] forward operand and [total] bias; re-homes the per-layer packed operands into one buffer on first use
        (or after a parameter was replaced) and refreshes the gathered bias when a parameter changed."""
        dev = self.linears[0].weight.device
        if self.wcat is None or self.wcat.device != dev:
            self.wcat = torch.empty((self.total, self.K), device=dev, dtype=_f32)
            self.bcat = torch.empty((self.total,), device=dev, dtype=_f32)
            self.wcat_t = self.t_table = None
            self.sig = self.sig_t = self.bias_table = None
        sig = _pack_epoch
        for lin, o, n in zip(self.linears, self.offsets, self.widths):
            w, b = lin.weight, lin.bias
            ent = packed(w, b, 1, False)
            want = self.wcat.data_ptr() + 4 * o * self.K
            # (reading ent.fwd is also what keeps this layer's rows of wcat in the repack table: the grouped GEMM reads them every step)
            if ent.fwd.data_ptr() != want:                  # new entry (first use, load_state_dict, ...): move its operand in
                view = self.wcat[o:o + n]
                view.copy_(ent.fwd)
                ent.fwd = view
                ent.fwd16 = None
                _invalidate_pack_table()                    # the repack table must learn the new destination
                self.sig = None
            sig += w._version + b._version + (w.data_ptr() ^ b.data_ptr())
        if sig != self.sig:
            if self.bias_table is None or self.bias_rows != [l.bias.data_ptr() for l in self.linears]:
                self.bias_rows = [l.bias.data_ptr() for l in self.linears]
                rows, begin = [], 0
                for lin, o, n in zip(self.linears, self.offsets, self.widths):
                    blocks = (n + _UT_ITEMS - 1) // _UT_ITEMS
                    rows.append([lin.bias.data_ptr(), self.bcat.data_ptr() + 4 * o, n, 1, 1, 1, 0, 0, 0, begin, 0, 0])
                    begin += blocks
                self.bias_table = (torch.tensor(rows, dtype=torch.int64).to(dev), len(rows), begin)
            t, n_rows, blocks = self.bias_table
            call("adm_unpack_wgrad_table", ptr(t), n_rows, blocks)       # (as a gather: accumulate = 0, zero_src = 0)
            self.sig = sig
        return self.wcat, self.bcat

    def transposed(self):
        """[K][total] operand of the embedding-gradient GEMM, refreshed when the weights changed."""
        if self.wcat_t is None:
            self.wcat_t = torch.empty((self.K, self.total), device=self.wcat.device, dtype=_f32)
            self.sig_t = self.t_table = None
        if self.sig_t != self.sig:
            # the LDS-tiled table kernel with ONE row: the [total][K] operand as the source of the [K][total] data-gradient image alone
            # (PT_FWD = 0; adm_pack_weight's element-wise transpose: 0.50 ms; this: ~0.09)
            if self.t_table is None:
                ent = _Packed()       # (no images; total and K are multiples of 32, so the row's padded sizes are the sizes themselves)
                ent.fwd, ent.bwd = self.wcat, self.wcat_t
                row = _pack_row(self.wcat, ent, self.total, self.K, 1, False, 0)
                row[PT_FWD] = 0
                self.t_table = torch.tensor([row], dtype=torch.int64).to(self.wcat.device)
            call("adm_pack_weight_table", ptr(self.t_table), 1, (self.total // 32) * (self.K // 32))
            self.sig_t = self.sig
        return self.wcat_t


class _AffineGroupFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, grp, *params):
        emb = _chk(emb, "emb")
        B, K = emb.shape
        if K != grp.K:
            raise RuntimeError(f"affine_group: embedding has {K} channels, the Linears expect {grp.K}")
        wcat, bcat = grp.operands()
        out = _new((B, grp.total), emb)
        with _Prof("igemm", 2.0 * B * grp.total * K, f"fwd-affine-group M={B} N={grp.total} K={K}"):
            call("adm_conv_fwd", ptr(emb), ptr(wcat), ptr(bcat), None, ptr(out), B, 1, 1, K, K, grp.total, grp.total, grp.total,
                 grp.total, 1, 0, -1)
        ctx.save_for_backward(emb)
        ctx.grp = grp
        ctx.set_materialize_grads(False)
        need = any(ctx.needs_input_grad)            # (grad mode is off inside forward(): ask the node, not torch.is_grad_enabled())
        # one gradient buffer for all blocks: block i's GroupNorm backward writes d scale/shift into columns [o_i, o_i + 2 C_i) itself
        # (ops._GroupNormAct finds its slot on the scale/shift tensor it was given) and hands autograd nothing for that edge
        ctx.dss = _new((B, grp.total), emb) if need else None
        ctx.flags = [[False] for _ in grp.widths]
        grp._last = (ctx.dss, ctx.flags)              # picked up by affine_group() right after apply()
        ctx.n_params = len(params)
        for i, p in enumerate(params):
            _mark_uses(ctx, (2 + i, p))
        return tuple(out[:, o:o + n] for o, n in zip(grp.offsets, grp.widths))

    @staticmethod
    def backward(ctx, *grads):
        (emb,) = ctx.saved_tensors
        grp, dss = ctx.grp, ctx.dss
        B, K = emb.shape
        T = grp.total
        # normally every slot was written by a GroupNorm backward and autograd delivers nothing; a gradient that did arrive through
        # autograd (some other consumer of a slice) is added to its slot, a slot nobody wrote is zero
        if any(g is not None for g in grads) or not all(f[0] for f in ctx.flags):
            for (o, n), g, f in zip(zip(grp.offsets, grp.widths), grads, ctx.flags):
                view = dss[:, o:o + n]
                if g is not None and f[0]:
                    view.add_(g)
                elif g is not None:
                    view.copy_(g)
                elif not f[0]:
                    view.zero_()
        if _branch_stream is not None:       # slots written by the second decoder's GroupNorm nodes on their own stream: autograd
            torch.cuda.current_stream().wait_stream(_branch_stream)      # orders streams only along edges that carry a tensor
        demb = None
        if ctx.needs_input_grad[0]:
            wt = grp.transposed()
            demb = _new((B, K), emb)
            sk = hip.lib().adm_conv_splitk(B, K, T)
            ws = _new((sk * B * K,), emb) if sk > 1 else None
            with _Prof("igemm", 2.0 * B * T * K, f"dgrad-affine-group M={B} N={K} K={T}"):
                call("adm_conv_fwd_ws", ptr(dss), ptr(wt), None, None, ptr(demb), ptr(ws), 0 if ws is None else ws.numel(), B, 1, 1, T, T, K,
                     K, K, K, 1, 0)
        params = [p for lin in grp.linears for p in (lin.weight, lin.bias)]
        need_w = any(ctx.needs_input_grad[2:])
        out = [None] * ctx.n_params
        if need_w:
            sinks = [_direct_grad(p) for p in params]
            direct = all(s is not None for s in sinks) and DEFER_UNPACK and not DETERMINISTIC
            if direct:
                _begin_defer()
                if grp.ws_w is None or grp.ws_w.device != emb.device:
                    grp.ws_w = torch.zeros((T, K), device=emb.device, dtype=_f32)
                    grp.ws_b = torch.zeros((T,), device=emb.device, dtype=_f32)
                    _rest_ws[("affine_group", id(grp), "w")] = grp.ws_w      # (re-zeroed with the others after a pass that raised)
                    _rest_ws[("affine_group", id(grp), "b")] = grp.ws_b
                if grp.ws_w.data_ptr() in _unpack_pending:
                    flush_deferred_unpack()
                dwp, dbp, auto = grp.ws_w, grp.ws_b, -1
            else:
                dwp, dbp, auto = _new((T, K), emb), torch.zeros((T,), device=emb.device, dtype=_f32), 0
            with _Prof("wgrad", 2.0 * B * T * K, f"wgrad-affine-group P={B} Co={T} Ci={K}"):
                call("adm_conv_wgrad_bias", ptr(emb), ptr(dss), ptr(dwp), ptr(dbp), B, 1, 1, K, K, T, T, 1, 0, auto)
            for i, (lin, o, n) in enumerate(zip(grp.linears, grp.offsets, grp.widths)):
                if direct:
                    _defer_unpack(dwp[o:o + n], sinks[2 * i], n, K, 1, K, False)
                    _defer_unpack(dbp[o:o + n], sinks[2 * i + 1], n, 1, 1, 1, False)
                    _notify(lin.weight); _notify(lin.bias)
                else:      # the packed [2C][E] tile of a 1x1 layer IS its [out, in] gradient
                    out[2 * i], out[2 * i + 1] = dwp[o:o + n], dbp[o:o + n]
        return (demb, None, *out)


def affine_group(emb, grp: AffineGroup):
    """(scale/shift of block 0, of block 1, ...) = all the group's Linears applied to emb [B, E]; each result is a column slice
    [B, 2C] (row stride = sum of all widths) that ops.group_norm_act reads in place."""
    params = [p for lin in grp.linears for p in (lin.weight, lin.bias)]
    outs = _AffineGroupFn.apply(emb, grp, *params)
    dss, flags = grp._last
    grp._last = None
    if dss is not None:
        for v, o, n, f in zip(outs, grp.offsets, grp.widths, flags):
            v._adm_dss = (dss[:, o:o + n], f)          # (gradient slot, its "written" mark): ops.group_norm_act hands them to its node
    return outs


# ------------------------------------------------------------------------------------------------
# attention core
# ------------------------------------------------------------------------------------------------
ATTN_H3 = os.environ.get("ADM_ATTN_H3", "1") != "0"      # attention forward on the fp16 split format where qkv came with a bound
ATTN_H3_BWD = os.environ.get("ADM_ATTN_H3_BWD", "1") != "0"      # ... and the backward, where dout came with one too


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads, amax=None):
        qkv = _chk(qkv, "qkv")
        B, H, W, C3 = qkv.shape
        L = H * W
        if C3 != heads * 192:
            raise RuntimeError(f"qkv has {C3} channels, expected {heads * 192}")
        out = _new((B, H, W, heads * 64), qkv)
        lse = _new((B * heads, L), qkv)
        # (not _fp16_format(): this kernel has no bf16 twin, so a qkv that came with a bound runs on it whatever BF16X6 says)
        h3 = amax is not None and ATTN_H3 and FP16X3 and COMPUTE == "f32" and (L in (32, 64, 128, 256) or (L % 256 == 0 and L <= 16384))
        with _Prof("attnh3" if h3 else "attn", 4.0 * L * L * 64 * B * heads):
            if h3:
                _check_bound(qkv, amax, "qkv (attention forward)")
                call("adm_attn_fwd_h3", ptr(qkv), ptr(out), ptr(lse), _bptr(amax), B, L, heads)
            else:
                call("adm_attn_fwd", ptr(qkv), ptr(out), ptr(lse), B, L, heads)
        ctx.save_for_backward(qkv, out, lse)
        ctx.heads = heads
        ctx.amax_qkv = amax if h3 else None
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        dout = _chk(dout, "dout")
        B, H, W, _ = qkv.shape
        dqkv = _like(qkv)
        delta = _like(lse)
        slot_a = _amax_slot(qkv) if (_fp16_format() and H3_GEMM) else None     # max |dqkv| for the qkv conv's gradients
        amax_g = _get_amax(dout) if (ctx.amax_qkv is not None and ATTN_H3_BWD) else None
        with _Prof("attnh3" if amax_g is not None else "attn", 10.0 * (H * W) ** 2 * 64 * B * ctx.heads):
            if amax_g is not None:      # both bounds at hand: the fp16 split format (attention_h3.hip)
                _check_bound(qkv, ctx.amax_qkv, "qkv (attention backward)")
                call("adm_attn_bwd_h3", ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(dqkv), ptr(delta), _bptr(ctx.amax_qkv), _bptr(amax_g),
                     ptr(slot_a), B, H * W, ctx.heads)
            elif slot_a is not None:
                call("adm_attn_bwd_amax", ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(dqkv), ptr(delta), ptr(slot_a), B, H * W, ctx.heads)
            else:
                call("adm_attn_bwd", ptr(qkv), ptr(out), ptr(dout), ptr(lse), ptr(dqkv), ptr(delta), B, H * W, ctx.heads)
        _reg_amax(dqkv, slot_a)
        return dqkv, None, None


def attention(qkv, heads: int):
    a = getattr(qkv, "_adm_amax", None)
    out = _Attention.apply(qkv, heads, a)
    if a is not None:
        out._adm_amax = a            # rows of softmax(q k^T) v are convex combinations of rows of v: |out| <= max |v| <= max |qkv|
    return out


# ------------------------------------------------------------------------------------------------
# resampling, concat, activation
# ------------------------------------------------------------------------------------------------
class _Resample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mode):
        x = _chk(x, "x")
        B, H, W, C = x.shape
        y = _new((B, H // 2, W // 2, C) if mode == 0 else (B, 2 * H, 2 * W, C), x)
        call("adm_resample2x", ptr(x), ptr(y), B, H, W, C, mode, 0.25 if mode == 0 else 1.0, 0)
        ctx.mode = mode
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _chk(dy, "dy")
        B, H, W, C = dy.shape
        if ctx.mode == 0:      # d(mean 2x2) = up * .25
            dx = _new((B, 2 * H, 2 * W, C), dy)
            call("adm_resample2x", ptr(dy), ptr(dx), B, H, W, C, 1, 0.25, 0)
            _reg_amax(dx, _get_amax(dy))
        else:                  # d(nearest x2) = 2x2 sum
            dx = _new((B, H // 2, W // 2, C), dy)
            call("adm_resample2x", ptr(dy), ptr(dx), B, H, W, C, 0, 1.0, 0)
        return dx, None


def downsample2x(x):
    y = _Resample.apply(x, 0)
    a = getattr(x, "_adm_amax", None)
    if a is not None:
        y._adm_amax = a              # a 2x2 mean is bounded by the bound of its inputs
    return y


def upsample2x(x):
    return _Resample.apply(x, 1)


class _Concat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, scale_b):
        a, b = _chk(a, "a"), _chk(b, "b")
        ca, cb = a.shape[-1], b.shape[-1]
        M = a.numel() // ca
        y = _new((*a.shape[:-1], ca + cb), a)
        slot = _amax_slot(a) if (_fp16_format() and H3_GEMM) else None
        # one launch for both halves; the concatenation feeds a block's 1x1 skip conv: the copy leaves the bound of what it wrote
        call("adm_concat2", ptr(a), ca, ptr(b), cb, ptr(y), M, float(scale_b), ptr(slot))
        if slot is not None:
            y._adm_amax = slot
        ctx.meta = (ca, cb, scale_b)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _chk(dy, "dy")
        ca, cb, scale_b = ctx.meta
        M = dy.numel() // (ca + cb)
        da = _new((*dy.shape[:-1], ca), dy)
        db = _new((*dy.shape[:-1], cb), dy)
        call("adm_split2", ptr(dy), ptr(da), ca, ptr(db), cb, M, float(scale_b))
        bound = _get_amax(dy)            # max |da|, max |db| <= max |dy| (scale_b <= 1)
        if bound is not None:
            _reg_amax(da, bound)
            if abs(scale_b) <= 1.0:
                _reg_amax(db, bound)
        return da, db, None


class _Fanout(torch.autograd.Function):
    """x -> n aliases of x, one per consumer; backward = ONE kernel summing the gradients that arrived (autograd would add them
    pairwise with its own elementwise kernels: two launches and six tensor passes for three consumers instead of one and four)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        gs = [_chk(g, "gradient") for g in grads if g is not None]
        if not gs:
            return None, None
        acc = gs[0]                      # (a single gradient passes through with whatever bound its producer registered)
        i = 1
        while i < len(gs):
            c = gs[i + 1] if i + 1 < len(gs) else None
            out = _like(acc)
            if acc.numel() % 4 == 0:
                last = i + 2 >= len(gs)
                slot_a = _amax_slot(acc) if (last and _fp16_format()) else None
                call("adm_add3", ptr(acc), ptr(gs[i]), ptr(c), ptr(out), ptr(slot_a), acc.numel())
                _reg_amax(out, slot_a)
                i += 2
            else:
                call("adm_add", ptr(acc), ptr(gs[i]), ptr(out), acc.numel())
                i += 1
            acc = out
        return acc, None


def fanout(x, n: int):
    """n aliases of x for n consumers (the gradient sum is one HIP launch); without a graph to record, x itself n times."""
    if n <= 1 or not (torch.is_grad_enabled() and x.requires_grad):
        return (x,) * max(n, 1)
    outs = _Fanout.apply(x, n)
    a = getattr(x, "_adm_amax", None)
    if a is not None:
        for o in outs:
            o._adm_amax = a          # (aliases of x)
    return outs


def concat_channels(a, b, scale_b: float = 1.0):
    return _Concat.apply(a, b, scale_b)


class _Silu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _chk(x, "x")
        y = _like(x)
        call("adm_silu_fwd", ptr(x), ptr(y), x.numel())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = _chk(dy, "dy")
        dx = _like(x)
        call("adm_silu_bwd", ptr(x), ptr(dy), ptr(dx), x.numel())
        return dx


def silu(x):
    return _Silu.apply(x)


def pos_embedding(t: torch.Tensor, channels: int) -> torch.Tensor:
    t = _chk(t.reshape(-1), "noise_labels")
    emb = _new((t.shape[0], channels), t)
    call("adm_pos_embedding", ptr(t), ptr(emb), t.shape[0], channels)
    return emb


# ------------------------------------------------------------------------------------------------
# SpatialAtt gate (+ the decouple residual)
# ------------------------------------------------------------------------------------------------
class _SpatialAtt(torch.autograd.Function):
    @staticmethod
    def forward(ctx, att, qk, h, xres):
        att, qk, h, xres = _chk(att, "att"), _chk(qk, "qk"), _chk(h, "h"), _chk(xres, "xres")
        B, H, W, C = h.shape
        y = _like(h)
        call("adm_spatial_att_fwd", ptr(att), att.shape[-1], ptr(qk), ptr(h), ptr(xres), ptr(y), B, H * W, C)
        ctx.save_for_backward(att, qk, h)
        return y

    @staticmethod
    def backward(ctx, dy):
        att, qk, h = ctx.saved_tensors
        dy = _chk(dy, "dy")
        B, H, W, C = h.shape
        dh = _like(h)
        datt = _like(att)
        dqk = torch.zeros_like(qk)
        part = _new((B, 4), h)           # per-image partials, summed in image order (no atomics: reproducible)
        call("adm_spatial_att_bwd", ptr(att), att.shape[-1], ptr(qk), ptr(h), ptr(dy), ptr(dh), ptr(datt), ptr(dqk), ptr(part),
             B, H * W, C)
        return datt, dqk, dh, dy


def spatial_att_gate(att, qk, h, xres):
    """softsign(softmax-pooled att) * h + xres; att = `map` conv output (channel 0 of a 32-padded tensor)."""
    return _SpatialAtt.apply(att, qk, h, xres)


# ------------------------------------------------------------------------------------------------
# layout + preconditioning
# ------------------------------------------------------------------------------------------------
def _nchw_to_nhwc(x, mul, cpad):
    B, C, H, W = x.shape
    y = _new((B, H, W, cpad), x)
    bs = 0 if (mul is None or mul.numel() == 1) else 1
    slot = _amax_slot(x) if _fp16_format() else None
    if slot is not None:        # the UNet's input with its bound: the stem conv and its weight gradient run on the fp16 format
        call("adm_nchw_to_nhwc_amax", ptr(x), int(x.dtype == torch.float64), ptr(mul), bs, ptr(y), ptr(slot), B, C, H * W, cpad)
        y._adm_amax = slot
    else:
        call("adm_nchw_to_nhwc", ptr(x), int(x.dtype == torch.float64), ptr(mul), bs, ptr(y), B, C, H * W, cpad)
    return y


class _NchwToNhwc(torch.autograd.Function):
    """The stem's layout change fused with c_in * x (uncond_unet.py:627-628), differentiable in x: EDMPrecond.forward returns
    tensors that take part in autograd w.r.t. its input (uncond_unet.py:614-635; guidance-style callers differentiate through the
    denoiser).  Backward = the scaled NHWC -> NCHW transpose of the stem conv's data gradient."""

    @staticmethod
    def forward(ctx, x, mul, cpad):
        ctx.save_for_backward(mul)
        ctx.meta = (tuple(x.shape), x.dtype)
        return _nchw_to_nhwc(x, mul, cpad)

    @staticmethod
    def backward(ctx, dy):
        (mul,) = ctx.saved_tensors
        (B, C, H, W), dt = ctx.meta
        dy = _chk(dy, "dy")
        if mul is None:
            mul = torch.ones(1, device=dy.device, dtype=_f32)
        dx = _new((B, C, H, W), dy)
        call("adm_precond_out", None, 0, ptr(dy), dy.shape[-1], None, ptr(mul), 0 if mul.numel() == 1 else 1, ptr(dx), B, C, H * W)
        return (dx if dt == _f32 else dx.to(dt)), None, None


def nchw_to_nhwc(x: torch.Tensor, mul: Optional[torch.Tensor], cpad: int) -> torch.Tensor:
    """[B,C,H,W] fp32/fp64 -> [B,H,W,cpad] fp32 scaled per batch by ``mul`` ([B] or [1])."""
    hip.require_cuda(x, "x")
    if x.dtype not in (torch.float32, torch.float64):
        x = x.to(torch.float32)
    x = x if x.is_contiguous() else x.contiguous()
    if torch.is_grad_enabled() and x.requires_grad:
        return _NchwToNhwc.apply(x, None if mul is None else mul.detach(), cpad)
    return _nchw_to_nhwc(x, mul, cpad)


class _PrecondOut(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, x, a, s):
        f = _chk(f, "F")
        B, H, W, ldf = f.shape
        C = x.shape[1]
        out = _new((B, C, H, W), f)
        cbs = 0 if a.numel() == 1 else 1
        call("adm_precond_out", ptr(x), int(x.dtype == torch.float64), ptr(f), ldf, ptr(a), ptr(s), cbs, ptr(out), B, C,
             H * W)
        ctx.save_for_backward(s, a)
        ctx.meta = (ldf, C, cbs, x.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        s, a = ctx.saved_tensors
        ldf, C, cbs, xdt = ctx.meta
        dout = _chk(dout, "dout")
        B, _, H, W = dout.shape
        df = dx = None
        if ctx.needs_input_grad[0]:
            df = _new((B, H, W, ldf), dout)
            slot = _amax_slot(dout) if _fp16_format() else None
            if slot is not None:    # the output conv's dy with its bound: its data and weight gradients run on the fp16 format
                call("adm_precond_out_bwd_amax", ptr(dout), ptr(s), cbs, ptr(df), ldf, ptr(slot), B, C, H * W)
                _reg_amax(df, slot)
            else:
                call("adm_precond_out_bwd", ptr(dout), ptr(s), cbs, ptr(df), ldf, B, C, H * W)
        if ctx.needs_input_grad[1]:          # the skip path c_skip * x (uncond_unet.py:631-632)
            dx = _like(dout)
            call("adm_axpby_b", None, 0, ptr(dout), None, ptr(a), cbs, ptr(dx), B, dout.numel() // B)
            if xdt != _f32:
                dx = dx.to(xdt)
        return df, dx, None, None


def precond_out(f_nhwc, x_nchw, c_skip, c_out):
    """D = c_skip * x + c_out * F, NHWC(F) -> NCHW(D)."""
    return _PrecondOut.apply(f_nhwc, x_nchw, c_skip, c_out)


class _HeadOut(torch.autograd.Function):
    """NHWC (32-padded) -> NCHW of a head without preconditioning and without a skip term: the K | C head of the linear-drift DDM
    (six channels).  Unlike _PrecondOut it never sees the network input.  Backward: the zero-padded transpose with the bound of df,
    so the head conv's data and weight gradients stay on the fp16 format."""

    @staticmethod
    def forward(ctx, f, C):
        f = _chk(f, "F")
        B, H, W, ldf = f.shape
        out = _new((B, C, H, W), f)
        call("adm_nhwc_to_nchw", ptr(f), ldf, ptr(out), B, C, H * W)
        ctx.meta = (ldf, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        ldf, C = ctx.meta
        dout = _chk(dout, "dout")
        B, _, H, W = dout.shape
        df = _new((B, H, W, ldf), dout)
        slot = _amax_slot(dout) if _fp16_format() else None
        call("adm_nhwc_to_nchw_bwd_amax", ptr(dout), ptr(df), ldf, ptr(slot), B, C, H * W)
        _reg_amax(df, slot)
        return df, None


def head_out(f_nhwc, channels: int):
    """F as NCHW [B,channels,H,W] from the NHWC head output (channels <= 8)."""
    return _HeadOut.apply(f_nhwc, int(channels))


class _AxpbyB(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, x, a, s):
        y = _chk(y, "y")
        B = y.shape[0]
        n = y.numel() // B
        out = _like(y)
        cbs = 0 if s.numel() == 1 else 1
        call("adm_axpby_b", ptr(x), int(x.dtype == torch.float64), ptr(y), ptr(a), ptr(s), cbs, ptr(out), B, n)
        ctx.save_for_backward(s, a)
        ctx.cbs, ctx.xdt = cbs, x.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        s, a = ctx.saved_tensors
        dout = _chk(dout, "dout")
        B = dout.shape[0]
        dy = dx = None
        if ctx.needs_input_grad[0]:
            dy = _like(dout)
            call("adm_axpby_b", None, 0, ptr(dout), None, ptr(s), ctx.cbs, ptr(dy), B, dout.numel() // B)
        if ctx.needs_input_grad[1]:
            dx = _like(dout)
            call("adm_axpby_b", None, 0, ptr(dout), None, ptr(a), ctx.cbs, ptr(dx), B, dout.numel() // B)
            if ctx.xdt != _f32:
                dx = dx.to(ctx.xdt)
        return dy, dx, None, None


def axpby_batch(y, x, a, s):
    """out = a[b] * x + s[b] * y (gradients flow to y, and to x when it requires one)."""
    return _AxpbyB.apply(y, x, a, s)


# ------------------------------------------------------------------------------------------------
# KL autoencoder (frozen first stage): forward-only helpers
# ------------------------------------------------------------------------------------------------
def _no_grad_only(*tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError("adm_amd: this op is forward-only (the first stage is frozen: ddm_const_2.py:436-440); "
                           "call it under torch.no_grad() with parameters that do not require grad")


# The strided / large-filter convs: ops.conv2d_strided here (forward-only), ops_ae._ConvDown and ops_cond._ConvGeneric with their
# backwards.  They differ in how the weight operand is made and in the weight-gradient kernel; what they share is below.
def _conv_fwd_strided(x, weight, wp, bp, stride, pad_lo, pad_hi, label):
    """y = conv(x) with filter size ks <= 7 from the OIHW `weight`, a stride and explicit zero padding (pad_lo rows/cols on the top/left,
    pad_hi on the bottom/right), on the packed operand wp and the packed bias bp; x is checked NHWC."""
    B, H, W, cx = x.shape
    co, ci, ks = weight.shape[0], weight.shape[1], weight.shape[-1]
    cop, cip = ceil32(co), ceil32(ci)
    if cx != cip:
        raise RuntimeError(f"conv input has {cx} channels, expected {cip}")
    Ho, Wo = (H + pad_lo + pad_hi - ks) // stride + 1, (W + pad_lo + pad_hi - ks) // stride + 1
    y = _new((B, Ho, Wo, cop), x)
    with _Prof("igemm", 2.0 * B * Ho * Wo * co * ci * ks * ks, f"{label} M={B * Ho * Wo} N={cop} K={ks * ks * cip}"):
        call("adm_conv_fwd_strided", ptr(x), ptr(wp), ptr(bp), None, ptr(y), B, H, W, Ho, Wo, cip, cip, cop, cop, cop, cop, ks, stride,
             pad_lo)
    return y


def _conv_dgrad_strided(dy, weight, x_shape, stride, pad_lo):
    """dx of the conv above as the transposed conv in GEMM form: col = dy x W^T on the 1x1 kernel, then the adm_col2im gather."""
    B, H, W, cip = x_shape
    Ho, Wo = dy.shape[1], dy.shape[2]
    co, ci, ks = weight.shape[0], weight.shape[1], weight.shape[-1]
    cop = ceil32(co)
    w = _chk(weight.detach(), "weight")
    wt = _new((ks * ks * cip, cop), dy)
    call("adm_pack_weight_tconv", ptr(w), ptr(wt), co, ci, ks, cop, cip)
    M = B * Ho * Wo
    col = _new((M, ks * ks * cip), dy)
    with _Prof("igemm", 2.0 * M * co * ci * ks * ks, f"dgrad-tconv M={M} N={ks * ks * cip} K={cop}"):
        call("adm_conv_fwd", ptr(dy), ptr(wt), None, None, ptr(col), 1, M, 1, cop, cop, ks * ks * cip, ks * ks * cip,
             ks * ks * cip, ks * ks * cip, 1, 0, -1)
    dx = _new((B, H, W, cip), dy)
    call("adm_col2im", ptr(col), ptr(dx), B, H, W, Ho, Wo, cip, ks, stride, pad_lo)
    return dx


def _conv_wgrad_strided(x, dy, weight, bias, need_b, stride, pad_lo, det_ok):
    """(dw, db) of the conv above for autograd, None where the flat gradient buffer took one; need_b: the bias wants a gradient.
    det_ok: under ADM_DETERMINISTIC=1 the pixel-range partials go to a workspace and are summed in split order (no float atomics)."""
    B, H, W, cip = x.shape
    Ho, Wo = dy.shape[1], dy.shape[2]
    co, ci, ks = weight.shape[0], weight.shape[1], weight.shape[-1]
    cop = ceil32(co)
    det = det_ok and DETERMINISTIC
    dbp = torch.zeros((cop,), device=dy.device, dtype=_f32) if need_b else None
    dwp, splits, bws = _wgrad_workspace("wgrad", det, False, weight, dy, B, Ho, Wo, cip, cop, ks, 0, 0, ks * ks, need_b)
    with _Prof("wgrad", 2.0 * B * Ho * Wo * co * ci * ks * ks, f"wgrad-k{ks}s{stride} P={B * Ho * Wo} Co={cop} Ci={cip}"):
        size = (B, H, W, Ho, Wo, cip, cip, cop, cop, ks, stride, pad_lo)
        if det:
            call("adm_conv_wgrad_strided_ws", ptr(x), ptr(dy), ptr(dwp), ptr(bws), *size, splits)
        else:
            call("adm_conv_wgrad_strided", ptr(x), ptr(dy), ptr(dwp), ptr(dbp), *size)
    sink = _direct_grad(weight)
    dw = _unpack_wgrad(weight, sink, dwp, ks, False, False, False, splits, bws, dbp)
    if sink is not None:
        _notify(weight)
    db = None
    if dbp is not None:          # the padded bias gradient: added into the flat gradient buffer, or its real entries for autograd
        bsink = _direct_grad(bias)
        if bsink is not None:
            call("adm_add", ptr(bsink), ptr(dbp), ptr(bsink), co)
            _notify(bias)
        else:
            db = dbp[:co].clone()
    return dw, db


def conv2d_strided(x, weight, bias=None, *, stride=2, pad_lo=0, pad_hi=1):
    """NHWC conv with a stride and explicit zero padding (pad_lo rows/cols on the top/left, pad_hi on the bottom/right).
    F.pad(x, (0,1,0,1)) + Conv2d(3x3, stride 2, padding 0) of the autoencoder's Downsample (encoder_decoder.py:78-96)
    is stride=2, pad_lo=0, pad_hi=1.  Forward-only."""
    _no_grad_only(x, weight, bias)
    x = _chk(x, "x")
    pk = packed(weight, bias, weight.shape[-1], False)
    return _conv_fwd_strided(x, weight, pk.fwd, pk.bias, stride, pad_lo, pad_hi, f"fwd-s{stride}")


def _mm_nt(a, b, bias, out):
    """The launch of matmul_nt, for callers that have checked their operands (ops_ae's attention core, with a backward of its own)."""
    M, K = a.shape
    N = b.shape[0]
    with _Prof("igemm", 2.0 * M * N * K, f"mm M={M} N={N} K={K}"):
        call("adm_conv_fwd", ptr(a), ptr(b), ptr(bias), None, ptr(out), 1, M, 1, K, K, N, N, N, N, 1, 0, -1)
    return out


def matmul_nt(a, b, bias=None, out=None):
    """out[M][N] = sum_k a[m][k] * b[n][k] (+ bias[n]) on the implicit-GEMM kernel (a 1x1 'conv' over M pixels whose
    weight matrix is b).  K % 32 == 0; rows 16-byte aligned.  Forward-only."""
    _no_grad_only(a, b, bias)
    a, b = _chk(a, "a"), _chk(b, "b")
    K = a.shape[1]
    if b.shape[1] != K or K % 32:
        raise RuntimeError(f"matmul_nt: inner sizes {K} / {b.shape[1]} must match and be a multiple of 32")
    return _mm_nt(a, b, bias, out if out is not None else _new((a.shape[0], b.shape[0]), a))


def softmax_rows_(s, scale: float):
    """In place: s[r] = softmax(scale * s[r]) over the last dim of a contiguous 2-D fp32 tensor."""
    hip.require_cuda(s, "s")
    rows, cols = s.shape
    call("adm_softmax_rows", ptr(s), rows, cols, cols, float(scale))
    return s


def posterior_sample(moments, C: int, eps=None, zscale: float = 1.0):
    """moments NHWC [B,H,W,>=2C] (mean | logvar) -> z NHWC [B,H,W,C] = zscale * (mean + std * eps); eps NHWC [B,H,W,C]
    or None for the mode (DiagonalGaussianDistribution, ddm/encoder_decoder.py:854-892)."""
    moments = _chk(moments, "moments")
    B, H, W, ld = moments.shape
    z = _new((B, H, W, C), moments)
    e = None if eps is None else _chk(eps, "eps")
    call("adm_posterior_sample", ptr(moments), ld, ptr(e), ptr(z), C, B * H * W, C, float(zscale))
    return z


# ------------------------------------------------------------------------------------------------
# analytic schedule
# ------------------------------------------------------------------------------------------------
def q_sample(x0, noise, t, schedule: int):
    x0, noise, t = _chk(x0, "x0"), _chk(noise, "noise"), _chk(t, "t")
    B = x0.shape[0]
    xt = _like(x0)
    call("adm_q_sample", ptr(x0), ptr(noise), ptr(t), ptr(xt), B, x0.numel() // B, schedule)
    return xt


class _DdmLoss(torch.autograd.Function):
    """loss = sum_b [w1 SSE(C_pred, -x0) + w2 SSE(noise_pred, noise)] / B ; also returns per-sample terms."""

    @staticmethod
    def forward(ctx, c_pred, n_pred, x0, noise, w):
        c_pred, n_pred = _chk(c_pred, "C_pred"), _chk(n_pred, "noise_pred")
        B = c_pred.shape[0]
        n = c_pred.numel() // B
        per = _new((B,), c_pred, torch.float64)          # the sums leave the kernel in fp64 and are rounded to f32 once
        dc, dn = _like(c_pred), _like(n_pred)
        call("adm_ddm_loss", ptr(c_pred), ptr(n_pred), ptr(x0), ptr(noise), ptr(w), ptr(per), ptr(dc), ptr(dn), 1.0 / B,
             B, n)
        per = per.to(_f32)
        ctx.save_for_backward(dc, dn)
        ctx.mark_non_differentiable(per)
        return per.sum() / B, per

    @staticmethod
    def backward(ctx, gloss, _gper):
        dc, dn = ctx.saved_tensors
        return dc * gloss, dn * gloss, None, None, None


def ddm_loss(c_pred, n_pred, x0, noise, w):
    return _DdmLoss.apply(c_pred, n_pred, _chk(x0, "x0"), _chk(noise, "noise"), _chk(w, "weights"))


class _DdmLossL1(torch.autograd.Function):
    """Pixel-space loss with use_l1 (ddm_const.py:343-348 / ddm_const_2.py:235-240): simple_b = [w1 (SSE_C + mean|e_C|) +
    w2 (SSE_eps + mean|e_eps|)] / 2.  Returns (sum_b simple_b / B, per-sample simple); the four fp64 sums of the kernel are
    combined here in fp64 and rounded to f32 once."""

    @staticmethod
    def forward(ctx, c_pred, n_pred, x0, noise, w):
        c_pred, n_pred = _chk(c_pred, "C_pred"), _chk(n_pred, "noise_pred")
        B = c_pred.shape[0]
        n = c_pred.numel() // B
        sums = _new((B, 4), c_pred, torch.float64)
        dc, dn = _like(c_pred), _like(n_pred)
        call("adm_ddm_loss_l1", ptr(c_pred), ptr(n_pred), ptr(x0), ptr(noise), ptr(w), ptr(sums), ptr(dc), ptr(dn), 1.0 / B,
             B, n)
        w64 = w.to(torch.float64)
        per = (0.5 * (w64[:, 0] * (sums[:, 0] + sums[:, 2] / n) + w64[:, 1] * (sums[:, 1] + sums[:, 3] / n))).to(_f32)
        ctx.save_for_backward(dc, dn)
        ctx.mark_non_differentiable(per)
        return per.sum() / B, per

    @staticmethod
    def backward(ctx, gloss, _gper):
        dc, dn = ctx.saved_tensors
        return dc * gloss, dn * gloss, None, None, None


def ddm_loss_l1(c_pred, n_pred, x0, noise, w):
    """The pixel-space p_losses with use_l1: like ddm_loss, with the per-sample MEAN absolute errors added and the sum halved.
    w = [B][2] as DDPMBase.loss_weights makes it ('const' and 'const_2' alike)."""
    return _DdmLossL1.apply(c_pred, n_pred, _chk(x0, "x0"), _chk(noise, "noise"), _chk(w, "weights"))


class _DdmLossLatent(torch.autograd.Function):
    """LatentDiffusion.p_losses (ddm_const_2.py:527-596): weighted SSE + w3 * sum|x_rec - x0|.  Returns
    (sum_b simple_b / B, per-sample simple, per-sample un-weighted L1)."""

    @staticmethod
    def forward(ctx, c_pred, n_pred, x0, noise, xt, t, w, schedule, use_l1):
        c_pred, n_pred = _chk(c_pred, "C_pred"), _chk(n_pred, "noise_pred")
        B = c_pred.shape[0]
        n = c_pred.numel() // B
        per, l1 = _new((B,), c_pred, torch.float64), _new((B,), c_pred, torch.float64)      # (fp64 sums, rounded to f32 once)
        dc, dn = _like(c_pred), _like(n_pred)
        call("adm_ddm_loss_latent", ptr(c_pred), ptr(n_pred), ptr(x0), ptr(noise), ptr(xt), ptr(t), ptr(w), ptr(per),
             ptr(l1), ptr(dc), ptr(dn), 1.0 / B, B, n, int(schedule), int(use_l1))
        per, l1 = per.to(_f32), l1.to(_f32)
        ctx.save_for_backward(dc, dn)
        ctx.mark_non_differentiable(per, l1)
        return (per.sum() + (l1 * w[:, 2]).sum()) / B, per, l1

    @staticmethod
    def backward(ctx, gloss, _gper, _gl1):
        dc, dn = ctx.saved_tensors
        return dc * gloss, dn * gloss, None, None, None, None, None, None, None


def ddm_loss_latent(c_pred, n_pred, x0, noise, xt, t, w, schedule: int = 1, use_l1: bool = False):
    """schedule 0 = 'const' (x_rec uses sqrt(t) eps), 1 = 'const_2' (t eps); use_l1 adds the L1 twins of both SSE terms and
    halves the sum (ddm_const_2.py:556-559)."""
    return _DdmLossLatent.apply(c_pred, n_pred, _chk(x0, "x0"), _chk(noise, "noise"), _chk(xt, "x_t"), _chk(t, "t"),
                                _chk(w, "weights"), int(schedule), bool(use_l1))


def sampler_step(x64, c_pred, n_pred, t_cur: float, t_next: float, schedule: int, clip_x0: bool, scale_input: float,
                 last: bool):
    call("adm_sampler_step", ptr(x64), ptr(_chk(c_pred, "C")), ptr(_chk(n_pred, "noise")), float(t_cur), float(t_next),
         schedule, int(clip_x0), float(scale_input), int(last), x64.numel())
    return x64


def sampler_step_stochastic(x64, c_pred, n_pred, z64, t64, s64, schedule: int, clip_x0: bool, scale_input: float,
                            last: bool):
    """In-place stochastic reverse step on the fp64 state (per-image t, s as fp64 device vectors)."""
    B = x64.shape[0]
    call("adm_sampler_step_stochastic", ptr(x64), ptr(_chk(c_pred, "C")), ptr(_chk(n_pred, "noise")), ptr(z64), ptr(t64),
         ptr(s64), schedule, int(clip_x0), float(scale_input), int(last), B, x64.numel() // B)
    return x64


# ------------------------------------------------------------------------------------------------
# linear-drift schedule (ddm/ddm_linear.py; csrc/ddm_linear.hip)
# ------------------------------------------------------------------------------------------------
def q_sample_linear(x0, noise, K, t):
    """x_t = x0 + K t^2/2 + C t + sqrt(t) eps, C = -x0 - K/2; K is clamped to [-1, 1] inside the kernel."""
    x0, noise, K, t = _chk(x0, "x0"), _chk(noise, "noise"), _chk(K, "K"), _chk(t, "t")
    B = x0.shape[0]
    xt = _like(x0)
    call("adm_q_sample_linear", ptr(x0), ptr(noise), ptr(K), ptr(t), ptr(xt), B, x0.numel() // B)
    return xt


class _DdmLossLinear(torch.autograd.Function):
    """ddm_linear.DDPM.p_losses without its LPIPS summand: returns (sum_b simple_b / B + sum_b w3_b MAE_b, per-sample simple,
    per-sample MAE); w = [B][3] = (w1, w2, w3) with w3 = mean_b (1 - t_b)^2 / B."""

    @staticmethod
    def forward(ctx, theta_pred, n_pred, x0, noise, K, xt, t, w, use_l1):
        theta_pred, n_pred = _chk(theta_pred, "theta_pred"), _chk(n_pred, "noise_pred")
        B = n_pred.shape[0]
        n3 = n_pred.numel() // B
        if theta_pred.numel() != 2 * B * n3:
            raise RuntimeError(f"theta_pred {tuple(theta_pred.shape)} must hold K_pred | C_pred of noise_pred {tuple(n_pred.shape)}")
        per, mae = _new((B,), n_pred), _new((B,), n_pred)
        dth, dn = _like(theta_pred), _like(n_pred)
        call("adm_ddm_loss_linear", ptr(theta_pred), ptr(n_pred), ptr(x0), ptr(noise), ptr(K), ptr(xt), ptr(t), ptr(w), ptr(per),
             ptr(mae), ptr(dth), ptr(dn), B, n3, int(use_l1))
        ctx.save_for_backward(dth, dn)
        ctx.mark_non_differentiable(per, mae)
        return per.sum() / B + (mae * w[:, 2]).sum(), per, mae

    @staticmethod
    def backward(ctx, gloss, _gper, _gmae):
        dth, dn = ctx.saved_tensors
        return dth * gloss, dn * gloss, None, None, None, None, None, None, None


def ddm_loss_linear(theta_pred, n_pred, x0, noise, K, xt, t, w, use_l1: bool = False):
    return _DdmLossLinear.apply(theta_pred, n_pred, _chk(x0, "x0"), _chk(noise, "noise"), _chk(K, "K"), _chk(xt, "x_t"),
                                _chk(t, "t"), _chk(w, "weights"), bool(use_l1))


def sampler_step_linear(x32, theta_pred, n_pred, z32, t32, s32, scale_input: float, last: bool):
    """In-place reverse step of the linear-drift sampler on the fp32 state (per-image t, s as fp32 device vectors)."""
    B = x32.shape[0]
    if not x32.is_contiguous():
        raise RuntimeError("adm_amd: the sampler state is updated in place and must be contiguous")
    call("adm_sampler_step_linear", ptr(_chk(x32, "x")), ptr(_chk(theta_pred, "theta_pred")), ptr(_chk(n_pred, "noise")),
         ptr(_chk(z32, "z")), ptr(_chk(t32, "t")), ptr(_chk(s32, "s")), float(scale_input), int(last), B, x32.numel() // B)
    return x32


# ------------------------------------------------------------------------------------------------
# LPIPS branch of the pixel-space loss (csrc/lpips.hip; the VGG16 convolutions themselves are conv2d)
# ------------------------------------------------------------------------------------------------
class _LpipsInput(torch.autograd.Function):
    """(x_rec - shift) / scale as NHWC with 32 channels, x_rec formed from the predictions in the same kernel:
    schedule -1 = `a` is the image itself, 0 = -C_pred, 1 = x_noisy - C_pred t - t noise_pred, 2 = the linear-drift schedule with
    a = theta_pred (six channels): x_noisy - K_pred t^2/2 - C_pred t - sqrt(t) noise_pred."""

    @staticmethod
    def forward(ctx, a, n_pred, x_noisy, t, shift, scale, schedule):
        a = _chk(a, "C_pred" if schedule >= 0 else "image")
        B, C, H, W = a.shape
        if C != (6 if schedule == 2 else 3):
            raise NotImplementedError("the LPIPS input has three channels (theta_pred of the linear schedule: six)")
        if schedule >= 1:
            n_pred, x_noisy, t = _chk(n_pred, "noise_pred"), _chk(x_noisy, "x_noisy"), _chk(t, "t")
        y = _new((B, H, W, 32), a)
        call("adm_lpips_input", ptr(a), ptr(n_pred), ptr(x_noisy), ptr(t), ptr(shift), ptr(scale), ptr(y), B, H * W, schedule)
        ctx.save_for_backward(t if schedule >= 1 else None, scale)
        ctx.meta = (tuple(a.shape), schedule)
        return y

    @staticmethod
    def backward(ctx, dy):
        t, scale = ctx.saved_tensors
        (B, C, H, W), schedule = ctx.meta
        dy = _chk(dy, "dy")
        da = _new((B, C, H, W), dy)
        dn = _new((B, 3, H, W), dy) if schedule >= 1 else None
        call("adm_lpips_input_bwd", ptr(dy), ptr(t), ptr(scale), ptr(da), ptr(dn), B, H * W, schedule)
        return da, dn, None, None, None, None, None


class _LpipsInputC1(torch.autograd.Function):
    """_LpipsInput for a one-channel image [B,1,H,W]: ScalingLayer's broadcast (lpips.py:56-63) fills channels 0..2 from the one x_rec;
    the gradient is the sum over the three channels in a fixed order.  Schedules -1, 0 and 1."""

    @staticmethod
    def forward(ctx, a, n_pred, x_noisy, t, shift, scale, schedule):
        a = _chk(a, "C_pred" if schedule >= 0 else "image")
        B, _, H, W = a.shape
        if schedule == 1:
            n_pred, x_noisy, t = _chk(n_pred, "noise_pred"), _chk(x_noisy, "x_noisy"), _chk(t, "t")
            if n_pred.shape != a.shape or x_noisy.shape != a.shape:
                raise RuntimeError("adm_amd: noise_pred and x_noisy must be one-channel like C_pred")
        y = _new((B, H, W, 32), a)
        call("adm_lpips_input_c1", ptr(a), ptr(n_pred), ptr(x_noisy), ptr(t), ptr(shift), ptr(scale), ptr(y), B, H * W, schedule)
        ctx.save_for_backward(t if schedule == 1 else None, scale)
        ctx.meta = (tuple(a.shape), schedule)
        return y

    @staticmethod
    def backward(ctx, dy):
        t, scale = ctx.saved_tensors
        (B, _, H, W), schedule = ctx.meta
        dy = _chk(dy, "dy")
        da = _new((B, 1, H, W), dy)
        dn = _new((B, 1, H, W), dy) if schedule == 1 else None
        call("adm_lpips_input_c1_bwd", ptr(dy), ptr(t), ptr(scale), ptr(da), ptr(dn), B, H * W, schedule)
        return da, dn, None, None, None, None, None


def lpips_input(a, n_pred, x_noisy, t, shift, scale, schedule: int):
    """The LPIPS network's input [B,H,W,32] from NCHW tensors: schedule -1 takes the image `a`; 0 ('const') and 1 ('const_2')
    take a = C_pred and rebuild x_rec (ddm_const.py:326 / ddm_const_2.py:217); 2 ('linear') takes a = theta_pred [B,6,H,W]
    (ddm_linear.py:173-176).  Differentiable in a and, for const_2 and linear, n_pred.  A one-channel `a` takes the broadcasting
    kernel (schedules -1, 0, 1)."""
    if schedule not in (-1, 0, 1, 2):
        raise ValueError(schedule)
    one_channel = a.dim() == 4 and a.shape[1] == 1
    if one_channel and schedule == 2:
        raise NotImplementedError("the linear schedule's LPIPS input is not built for a one-channel image")
    shift, scale = _chk(shift.reshape(-1), "shift"), _chk(scale.reshape(-1), "scale")
    if schedule < 1:
        n_pred = x_noisy = t = None
    if one_channel:
        return _LpipsInputC1.apply(a, n_pred, x_noisy, t, shift, scale, int(schedule))
    return _LpipsInput.apply(a, n_pred, x_noisy, t, shift, scale, int(schedule))


class _MaxPool2x2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _chk(x, "x")
        B, H, W, C = x.shape
        y = _new((B, H // 2, W // 2, C), x)
        call("adm_maxpool2x2_fwd", ptr(x), ptr(y), B, H, W, C)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        B, H, W, C = x.shape
        dx = _like(x)
        call("adm_maxpool2x2_bwd", ptr(x), ptr(_chk(dy, "dy")), ptr(dx), B, H, W, C)
        return dx


def maxpool2x2(x):
    """nn.MaxPool2d(kernel_size=2, stride=2) on NHWC; ties give their gradient to the first maximum, as F.max_pool2d does."""
    if x.shape[1] % 2 or x.shape[2] % 2:
        raise NotImplementedError("maxpool2x2 needs even H and W")
    return _MaxPool2x2.apply(x)


class _LpipsHeads(torch.autograd.Function):
    """out[b] = sum_k mean_p sum_c lin_k[c] (f0_k / (|f0_k| + 1e-10) - f1_k / (|f1_k| + 1e-10))^2 over the taps k: one launch pair per tap,
    summed in tap order into one [B] vector.  Differentiable in the f0_k only."""

    @staticmethod
    def forward(ctx, n, *args):
        f0s = [_chk(f, "f0") for f in args[:n]]
        f1s = [_chk(f, "f1") for f in args[n:2 * n]]
        ws = [_chk(w.detach().reshape(-1), "lin weight") for w in args[2 * n:]]
        B = f0s[0].shape[0]
        out = _new((B,), f0s[0])
        for k, (f0, f1, w) in enumerate(zip(f0s, f1s, ws)):
            _, H, W, C = f0.shape
            if f1.shape != f0.shape or w.numel() != C:
                raise RuntimeError(f"LPIPS head {k}: f0 {tuple(f0.shape)}, f1 {tuple(f1.shape)}, lin {w.numel()}")
            part = _new((B * hip.lib().adm_lpips_head_blocks(H * W),), f0)
            call("adm_lpips_head_fwd", ptr(f0), ptr(f1), ptr(w), ptr(out), ptr(part), B, H * W, C, int(k > 0))
        ctx.save_for_backward(*f0s, *f1s, *ws)
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, dout):
        n, t = ctx.n, ctx.saved_tensors
        dout = _chk(dout, "dout")
        grads = []
        for k in range(n):
            if not ctx.needs_input_grad[1 + k]:
                grads.append(None)
                continue
            f0, f1, w = t[k], t[n + k], t[2 * n + k]
            B, H, W, C = f0.shape
            df0 = _like(f0)
            call("adm_lpips_head_bwd", ptr(f0), ptr(f1), ptr(w), ptr(dout), ptr(df0), B, H * W, C)
            grads.append(df0)
        return (None, *grads, *([None] * (2 * n)))


def lpips_heads(f0s, f1s, lins):
    """Per-sample LPIPS value [B] from the tapped NHWC feature maps of the input (f0s) and the target (f1s) and the `lin` weights."""
    f0s, f1s, lins = list(f0s), list(f1s), list(lins)
    if not (len(f0s) == len(f1s) == len(lins)) or not f0s:
        raise ValueError("lpips_heads needs one f0, f1 and lin weight per tap")
    return _LpipsHeads.apply(len(f0s), *f0s, *[f.detach() for f in f1s], *lins)
