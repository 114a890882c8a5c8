"""Geometries, modes, data and forms of the UNet attention sweep, shared by tests/test_attn_cases_host.py (CPU) and
tests/test_hip_attention_forms.py (GPU).  A plain helper like bf16_cases.py and gn_cases.py, not a conftest.

The two kernel families (csrc/attention.hip on the fp32 MFMA, csrc/attention_h3.hip on the fp16 split format) choose a compiled form
from the sequence length L = H W alone; adm_attn_form() is the function their entry points choose through, so form() below is what
runs.  Everything here is CPU fp32 and deterministic (oracle.fill.hash_tensor); do not modify what data() returns -- it is cached and
shared.
"""
import collections
import ctypes
import functools

import torch

from oracle import fill

import fp64ref

BAR_A = 1e-5                # tests/test_hip_accuracy.py: e_max against fp64, every path
F32_TORCH_CEILING = 5e-6    # what the plain fp32 torch restatement stays under on the peaked and stair data (test_attn_cases_host.py)

# mode -> (forward symbol, backward symbol).  How ops.attention is brought to each: tests/test_hip_attention_forms.py::_run.
MODES = {
    "f32": ("adm_attn_fwd", "adm_attn_bwd"),                    # no bound on qkv, FP16X3 off
    "f32+amax": ("adm_attn_fwd", "adm_attn_bwd_amax"),          # no bound on qkv; the backward raises the bound of dqkv
    "h3": ("adm_attn_fwd_h3", "adm_attn_bwd_h3"),               # bounds on qkv and dout
    "h3-fwd": ("adm_attn_fwd_h3", "adm_attn_bwd_amax"),         # a bound on qkv, none on dout: the f32 backward reads the h3 forward's out / lse
}
F32_MODES = ("f32", "f32+amax")
ALL_MODES = tuple(MODES)
FAMILY = {"adm_attn_fwd": 0, "adm_attn_bwd": 0, "adm_attn_bwd_amax": 0, "adm_attn_fwd_h3": 1, "adm_attn_bwd_h3": 2}

# L -> (B, H, W, heads): B <= 2, heads <= 3; heads > 1 and B > 1 both occur in each family (blockIdx.x / heads and % heads are live)
GEOM = {
    1: (2, 1, 1, 3),          # one key: softmax = 1, out = v
    9: (1, 3, 3, 2),          # partial tile of the 1-wave form: 23 masked keys, 23 lanes without a query
    25: (2, 5, 5, 1),
    32: (1, 4, 8, 3),         # the 1-wave form, exact
    64: (2, 8, 8, 2),
    96: (2, 8, 12, 1),        # 3 waves
    128: (1, 8, 16, 3),       # 4 waves; the h3 backward's one 128-row fill
    160: (1, 10, 16, 2),      # 5 waves
    192: (2, 12, 16, 1),      # 6 waves
    224: (1, 14, 16, 2),      # 7 waves
    256: (2, 16, 16, 2),      # 8 waves; the h3 backward's two 128-row fills
    288: (1, 16, 18, 2),      # chunked, 256 + 32: a last chunk of one wave's worth
    512: (2, 16, 32, 1),      # chunked, exactly two chunks
    576: (1, 24, 24, 2),      # chunked, 256 + 256 + 64
    768: (1, 24, 32, 2),      # chunked, three chunks
}
H3_L = (32, 64, 128, 256, 512, 768)
STAIR_GEOM = {512: (1, 16, 32, 2), 768: (2, 24, 32, 1), 1024: (1, 32, 32, 1)}
STAIRS = ((512, (0, 12)), (1024, (0, 10, 20, 30)), (1024, (30, 20, 10, 0)), (768, (0, 25, 5)))      # L, logit offset per 256-key chunk

Case = collections.namedtuple("Case", "geom kind offsets modes")      # geom = (B, H, W, heads); kind = hashed | peaked | stair


def _cases():
    out = [Case(g, "hashed", None, ALL_MODES if L in H3_L else F32_MODES) for L, g in GEOM.items()]
    # logits of spread ~3 (extremes past +-10): the softmax is a few keys wide; 25 and 288 put masked keys next to them
    out += [Case(GEOM[L], "peaked", None, ALL_MODES if L in H3_L else F32_MODES) for L in (25, 32, 128, 288)]
    out += [Case(STAIR_GEOM[L], "stair", offs, ALL_MODES) for L, offs in STAIRS]
    return out


CASES = _cases()


def seq_len(case):
    return case.geom[1] * case.geom[2]


def case_id(case):
    B, H, W, heads = case.geom
    tail = "" if case.offsets is None else "-" + ".".join(str(o) for o in case.offsets)
    return f"L{H * W}-B{B}-{H}x{W}-h{heads}-{case.kind}{tail}"


@functools.lru_cache(maxsize=None)
def data(case):
    """(qkv [B, H, W, heads 192], dout [B, H, W, heads 64]) of a case, CPU fp32.
    hashed: uniform in [-1, 1).  peaked: qkv uniform in [-3, 3).  stair: hashed, then channel 0 of every head's q is 8 and channel 0
    of its k is the offset of the key's 256-key chunk, so every logit of that chunk gains 8 offset / 8 = offset."""
    B, H, W, heads = case.geom
    tag = case_id(case)
    qkv = fill.hash_tensor((B, H, W, heads * 192), "attnforms.qkv." + tag, 3.0 if case.kind == "peaked" else 1.0)
    dout = fill.hash_tensor((B, H, W, heads * 64), "attnforms.g." + tag, 1.0)
    if case.kind == "stair":
        L = H * W
        assert L == 256 * len(case.offsets)
        offs = torch.tensor(case.offsets, dtype=torch.float32).repeat_interleave(256).reshape(1, H, W)
        for h in range(heads):
            qkv[..., h * 192] = 8.0
            qkv[..., h * 192 + 64] = offs
    return qkv, dout


@functools.lru_cache(maxsize=None)
def reference(case):
    """fp64 {"out": (ref, mag), "dqkv": (ref, mag)} of a case on the CPU; computed once and shared."""
    qkv, dout = data(case)
    return fp64ref.attention(qkv, case.geom[3], dout)


# Data on which each third of dqkv in turn holds max |dqkv| (the bound vector is one maximum over what two kernels store: a third left
# out of it goes unnoticed while another dominates).  Factors of (q, k, v): q and k trade a power of two, so the logits keep their
# bits; dq grows with k and v, dk with q and v, dv with neither.
BOUND_SCALES = {"dv": (1.0, 1.0, 1.0), "dq": (0.25, 4.0, 16.0), "dk": (4.0, 0.25, 16.0)}
BOUND_L = 64


@functools.lru_cache(maxsize=None)
def bound_data(which):
    """(qkv, dout, heads) of the hashed L = BOUND_L case with q, k, v scaled by BOUND_SCALES[which]."""
    case = next(c for c in CASES if c.kind == "hashed" and seq_len(c) == BOUND_L)
    qkv, dout = data(case)
    heads = case.geom[3]
    t = qkv.clone().reshape(*qkv.shape[:-1], heads, 3, 64)
    for i, s in enumerate(BOUND_SCALES[which]):
        t[..., i, :] *= s
    return t.reshape(qkv.shape), dout, heads


def third_maxima(dqkv, heads):
    """max |.| of the dq, dk and dv thirds of a dqkv tensor."""
    return dqkv.detach().abs().reshape(-1, heads, 3, 64).amax(dim=(0, 1, 3)).tolist()


def torch_f32(qkv, heads, dout):
    """The fp32 torch restatement: matmul / softmax / autograd on the layout of ops.attention.  {"out", "dqkv"}."""
    shp = qkv.shape
    B, L = shp[0], shp[1] * shp[2]
    x = qkv.detach().clone().requires_grad_(True)
    t = x.reshape(B, L, heads, 3, 64).permute(3, 0, 2, 1, 4)
    P = torch.softmax(torch.matmul(t[0], t[1].transpose(-1, -2)) / 8.0, dim=-1)
    out = torch.matmul(P, t[2]).permute(0, 2, 1, 3).reshape(*shp[:-1], heads * 64)
    (dqkv,) = torch.autograd.grad(out, x, dout)
    return {"out": out.detach(), "dqkv": dqkv}


@functools.lru_cache(maxsize=None)
def e32(case):
    """{"out": e_max, "dqkv": e_max} of the fp32 torch restatement against fp64 on the case's data (CPU)."""
    qkv, dout = data(case)
    got, ref = torch_f32(qkv, case.geom[3], dout), reference(case)
    return {n: fp64ref.errors(got[n], *ref[n])[0] for n in ("out", "dqkv")}


def limit(case, out):
    """The e_max a kernel is held to: bar A on hashed data; on peaked and stair data max(bar A, 2 x the fp32 torch restatement) -- the
    rule of GroupNorm's offset data and cond_cases.FALLBACK."""
    return BAR_A if case.kind == "hashed" else max(BAR_A, 2.0 * e32(case)[out])


# ------------------------------------------------------------------------------------------------ forms
def form(family, L):
    """(waves per workgroup, rows per LDS fill, grid.y, chunked) of adm_attn_form, or None where the family refuses L.
    family 0 = attention.hip, 1 = the h3 forward, 2 = the h3 backward."""
    from adm_amd import hip
    out = (ctypes.c_int * 4)()
    rc = hip.lib().adm_attn_form(family, L, out)
    assert rc in (0, -22), rc
    return tuple(out) if rc == 0 else None


def form_label(family, L):
    """Name of the compiled form and of the path through it that L takes: f32 single chunk '<n>w' ('-partial': L < 32, guarded rows and
    masked keys), f32 chunked '8w-chunked-exact' / '-ragged' (a short last chunk: zero-filled LDS, masked keys); h3 '<n>w' or
    '8w-chunked', the backward with its rows per LDS fill."""
    f = form(family, L)
    if f is None:
        return None
    w, rows, gy, chunked = f
    if family == 0:
        if chunked:
            return "f32:8w-chunked-" + ("exact" if L % rows == 0 else "ragged")
        return f"f32:{w}w" + ("-partial" if L < rows else "")
    return ("h3fwd:" if family == 1 else "h3bwd:") + f"{w}w" + ("-chunked" if chunked else "") + (f"/{rows}" if family == 2 else "")


def forms_reached():
    """{form label} the table runs: each mode's forward and backward symbol at the case's L."""
    return {form_label(FAMILY[sym], seq_len(c)) for c in CASES for m in c.modes for sym in MODES[m]}
