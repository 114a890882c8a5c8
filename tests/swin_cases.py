"""Cases, data, forms and fp32 restatements of the Swin encoder kernel sweep (csrc/swin.hip), shared by tests/test_swin_cases_host.py,
tests/test_fp64ref_swin_host.py (CPU) and tests/test_hip_swin_forms.py (GPU).  A plain helper like attn_cases.py, not a conftest.

The LayerNorm kernels choose a register form from the row width C alone (adm_ln_form), the stem kernels a lane layout from the width E
alone (adm_patch_embed_form); the launches choose through those two functions, so ln_form() / pe_form() below are what runs.  The block
counts of the backward launches are read off the workspace queries (one partial per wave / per workgroup).

Everything here is CPU and deterministic (oracle.fill.hash_tensor); do not modify what the data functions return -- it is cached and
shared.  The torch restatements take a `defect`: tests/test_fp64ref_swin_host.py shows that the bar of the GPU sweep rejects each.
"""
import collections
import ctypes
import functools

import torch
import torch.nn.functional as F

from oracle import fill

import fp64ref
import swin_ref as R
import swin_sci_ref as S

BAR_A = 1e-5                # e_max against fp64, every form
F32_TORCH_CEILING = 5e-6    # what plain fp32 torch stays under on the attention and stem cases (test_fp64ref_swin_host.py)
EPS = 1e-5
WIN = 7

# ------------------------------------------------------------------------------------------------ forms
LN_ROWS, LN_BWD_MAXBLOCKS = 4, 256          # waves per workgroup and the cap of the backward grid (csrc/swin.hip)
PE_WAVES, PE_PART, PE_BWD_MAXBLOCKS = 4, 19, 256


def _query(name, arg, n):
    from adm_amd import hip
    out = (ctypes.c_int * n)()
    rc = getattr(hip.lib(), name)(arg, out)
    assert rc in (0, -22), rc
    return tuple(out) if rc == 0 else None


def ln_form(C):
    """(NQ, float4 of the row in its last used trip) of adm_ln_form, or None where the kernels refuse C."""
    return _query("adm_ln_form", C, 2)


def ln_label(merge, C):
    """'plain' or 'merge' : NQ : 'whole' (the row fills every one of the NQ trips) or 'partial' (lanes past the row's end in the last
    used trip, or whole trips that are empty)."""
    nq, last = ln_form(C)
    whole = last == 64 and -(-C // 256) == nq
    return f"{'merge' if merge else 'plain'}:NQ{nq}:{'whole' if whole else 'partial'}"


def ln_bwd_blocks(M, C):
    """Workgroups of the LayerNorm backward: its workspace is one partial [2][C] per wave."""
    from adm_amd import hip
    return hip.lib().adm_ln_bwd_ws_floats(M, C) // (LN_ROWS * 2 * C)


def pe_form(E):
    """(G lanes per token, Q float4 per lane, E / 4) of adm_patch_embed_form, or None where the kernels refuse E."""
    return _query("adm_patch_embed_form", E, 3)


def pe_label(E):
    g, q, e4 = pe_form(E)
    return f"G{g}Q{q}:{'past' if g * q > e4 else 'exact'}"


def pe_tokens(geom):
    B, H, W = geom
    return B * (H // 4) * (W // 4)


def pe_token_groups(geom, E):
    return -(-pe_tokens(geom) // (64 // pe_form(E)[0]))


def pe_bwd_blocks(geom, E):
    """Workgroups of the stem backward: its workspace is one partial [19][E] per workgroup."""
    from adm_amd import hip
    B, H, W = geom
    return hip.lib().adm_patch_embed_ln_bwd_ws_floats(B, H, W, E) // (PE_PART * E)


# ------------------------------------------------------------------------------------------------ LayerNorm, plain and merged
LN_C = (32, 36, 96, 256, 260, 384, 512, 640, 768, 1024, 1536, 2044, 2048)
LN_CASES = [(M, C) for C in LN_C for M in (1, 3, 37)] + [(4099, 32), (4099, 260)]          # 4099 rows: past the 256-block cap
# (Cin = 64 is the one width at which the merged row fills the NQ = 1 form exactly)
MERGE_CASES = ([(2, 9, 11, Cin) for Cin in (8, 24, 64, 96, 128, 192, 256, 384, 512)]
               + [(2, H, W, Cin) for Cin in (24, 128) for H, W in ((1, 1), (1, 5), (5, 1), (3, 3), (4, 6))]
               + [(2, 91, 91, 8)])                                                                # 4232 output rows: capped
# the class of row i is LN_CLASSES[i % 8]; "const" only at row 7 (a later row of that slot is plain)
LN_CLASSES = ("plain", "+300", "-1000", "tiny", "300+1e-2u", "1e4u", "sparse", "const")


def merge_rows(case):
    B, H, W, _ = case
    return B * ((H + 1) // 2) * ((W + 1) // 2)


def row_classes(M):
    """{class: LongTensor of rows}."""
    out = {}
    for i in range(M):
        c = LN_CLASSES[i % 8]
        if c == "const" and i != 7:
            c = "plain"
        out.setdefault(c, []).append(i)
    return {c: torch.tensor(r) for c, r in out.items()}


def class_errors(got, ref, mag):
    """{class: (e_max, e_rms)} of row tensors [M, C] (any leading shape that flattens to M rows): fp64ref.errors over the rows of each
    class alone, so that the mag of one class (a sparse row's ~sqrt(C), a tiny row's rstd) never sets the scale for another."""
    C = ref.shape[-1]
    g, r, m = (t.reshape(-1, C) for t in (got, ref, mag))
    return {c: fp64ref.errors(g[rows.to(g.device)], r[rows.to(r.device)], m[rows.to(m.device)]) for c, rows in row_classes(r.shape[0]).items()}


def _class_rows(M, C, tag):
    """[M, C] fp32 rows by class: u uniform in [-1, 1); plain u; u + 300; u - 1000; 1e-3 u (the class on which eps decides); 300 +
    1e-2 u; 1e4 u; sparse (zeros, 2.5 at index 3, -40 at C - 1); constant 7."""
    u = fill.hash_tensor((M, C), tag, 1.0, torch.float64)
    x = u.clone()
    for c, rows in row_classes(M).items():
        if c == "+300":
            x[rows] = u[rows] + 300.0
        elif c == "-1000":
            x[rows] = u[rows] - 1000.0
        elif c == "tiny":
            x[rows] = 1e-3 * u[rows]
        elif c == "300+1e-2u":
            x[rows] = 300.0 + 1e-2 * u[rows]
        elif c == "1e4u":
            x[rows] = 1e4 * u[rows]
        elif c == "sparse":
            x[rows] = 0.0
            x[rows, 3] = 2.5
            x[rows, C - 1] = -40.0
        elif c == "const":
            x[rows] = 7.0
    return x.to(torch.float32)


def _ln_params(C, tag):
    w = (1.0 + fill.hash_tensor((C,), tag + ".w", 0.1, torch.float64)).to(torch.float32)
    b = fill.hash_tensor((C,), tag + ".b", 0.1, torch.float64).to(torch.float32)
    return w, b


@functools.lru_cache(maxsize=None)
def ln_data(case):
    """(x [M, C], w, b, dy [M, C]) fp32 of a plain case."""
    M, C = case
    tag = f"swinforms.ln.{M}.{C}"
    return (_class_rows(M, C, tag + ".x"),) + _ln_params(C, tag) + (fill.hash_tensor((M, C), tag + ".dy", 1.0),)


@functools.lru_cache(maxsize=None)
def merge_data(case):
    """(x [B, H, W, Cin], w, b [4 Cin], dy [B, Ho, Wo, 4 Cin]) fp32 of a merged case: the gathered rows are built by class and sent back
    through the gather (a position past an odd edge has no source: such a row holds zeros there whatever its class)."""
    B, H, W, Cin = case
    M, C = merge_rows(case), 4 * Cin
    tag = f"swinforms.merge.{B}.{H}.{W}.{Cin}"
    iy, ix, ci, _ = fp64ref.merge_index(H, W, Cin)
    Ho, Wo = iy.shape[0], ix.shape[1]
    xp = torch.zeros(B, 2 * Ho, 2 * Wo, Cin)
    xp[:, iy, ix, ci] = _class_rows(M, C, tag + ".x").reshape(B, Ho, Wo, C)
    return (xp[:, :H, :W].contiguous(),) + _ln_params(C, tag) + (fill.hash_tensor((B, Ho, Wo, C), tag + ".dy", 1.0),)


def merge_whole_rows(case):
    """bool [M]: the 2x2 cell of the output row lies inside the map."""
    B, H, W, Cin = case
    _, _, _, inside = fp64ref.merge_index(H, W, Cin)
    return inside.all(dim=-1).reshape(1, -1).expand(B, -1).reshape(-1)


def gathered(case, t):
    """A tensor in x's layout [B, H, W, Cin] as the rows [M, 4 Cin] the kernel normalises (zeros past the edge)."""
    B, H, W, Cin = case
    iy, ix, ci, _ = fp64ref.merge_index(H, W, Cin, t.device)
    xp = torch.zeros(B, 2 * iy.shape[0], 2 * ix.shape[1], Cin, dtype=t.dtype, device=t.device)
    xp[:, :H, :W] = t
    return xp[:, iy, ix, ci].reshape(-1, 4 * Cin)


@functools.lru_cache(maxsize=None)
def ln_reference(case):
    x, w, b, dy = ln_data(case)
    return fp64ref.layer_norm_affine(x, w, b, EPS, dy)


@functools.lru_cache(maxsize=None)
def merge_reference(case):
    x, w, b, dy = merge_data(case)
    return fp64ref.merge_layer_norm(x, w, b, EPS, dy)


LN_DEFECTS = ("eps dropped", "eps 1e-6", "variance divisor C-1")
MERGE_DEFECTS = ("quads in (dx, dy) order", "padded positions left out of the divisor")


def torch_ln(x, w, b, dy, dtype=torch.float32, defect=None, merge=False):
    """The torch restatement of LayerNorm (merge: of the 2x2 gather and LayerNorm(4 Cin)) in `dtype` with autograd: {"y", "dx", "dw",
    "db"}.  Without a defect it is swin_ref.layer_norm / swin_ref.merge_ln."""
    xx, ww, bb = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, w, b))
    eps = {"eps dropped": 0.0, "eps 1e-6": 1e-6}.get(defect, EPS)
    if merge:
        B, H, W, Cin = xx.shape
        xp = F.pad(xx, (0, 0, 0, W % 2, 0, H % 2))
        order = [(dy_, dx_) for dy_ in (0, 1) for dx_ in (0, 1)] if defect == MERGE_DEFECTS[0] else [(dy_, dx_) for dx_ in (0, 1) for dy_ in (0, 1)]
        g = torch.cat([xp[:, a::2, c::2] for a, c in order], dim=-1)
    else:
        g = xx
    C = g.shape[-1]
    if defect is None:
        y = R.layer_norm(g, ww, bb, EPS)
    else:
        n = float(C)
        if defect == MERGE_DEFECTS[1]:
            n = fp64ref.merge_index(x.shape[1], x.shape[2], x.shape[3])[3].to(dtype).sum(dim=-1)[None, :, :, None]
            mean = g.sum(dim=-1, keepdim=True) / n
            var = ((g - mean).square() * fp64ref.merge_index(x.shape[1], x.shape[2], x.shape[3])[3].to(dtype)).sum(dim=-1, keepdim=True) / n
        else:
            mean = g.mean(dim=-1, keepdim=True)
            var = (g - mean).square().sum(dim=-1, keepdim=True) / (n - 1 if defect == LN_DEFECTS[2] else n)
        y = (g - mean) / torch.sqrt(var + eps) * ww + bb
    dx, dw, db = torch.autograd.grad(y, (xx, ww, bb), dy.to(dtype))
    return {"y": y.detach(), "dx": dx, "dw": dw, "db": db}


# ------------------------------------------------------------------------------------------------ window attention
# (B, H, W, heads, (shift_h, shift_w)); C = 32 heads
ATTN_GEOM = [(B, H, W, heads, (s, s)) for B, H, W, _, heads, s in R.ATTN_CASES.values()] + [
    (1, 1, 1, 1, (3, 3)),           # one real token and 48 bias keys
    (3, 13, 8, 3, (2, 5)),          # C = 96, unequal shifts, 36 units: a multiple of the 4 per workgroup, more than one workgroup
    (1, 15, 7, 1, (3, 3)),          # three windows on one axis, the shift off on the other; 3 units: a workgroup with an idle wave
    (2, 6, 20, 2, (6, 1)),
]
ATTN_KINDS = ("hashed", "peaked", "table")
AttnCase = collections.namedtuple("AttnCase", "geom kind")
ATTN_CASES = [AttnCase(g, k) for g in ATTN_GEOM for k in ATTN_KINDS]


def attn_id(case):
    B, H, W, heads, (sh, sw) = case.geom
    return f"B{B}-{H}x{W}-h{heads}-s{sh}.{sw}-{case.kind}"


def attn_units(geom):
    B, H, W, heads, _ = geom
    return B * (-(-H // WIN)) * (-(-W // WIN)) * heads


def attn_padded(geom):
    return geom[1] % WIN != 0 or geom[2] % WIN != 0


@functools.lru_cache(maxsize=None)
def attn_data(case):
    """(qkv [B, H, W, 3C], qkv_bias [3C], table [169, heads], dout [B, H, W, C]) fp32.  hashed: qkv uniform in [-1, 1), the bias in
    [-0.5, 0.5), the table in [-0.5, 0.5).  peaked: qkv x 4 (logits past +-10: the softmax is a few keys wide).  table: the table in
    [-20, 20), qkv x 0.1 (the relative-position index decides the output)."""
    B, H, W, heads, _ = case.geom
    C = 32 * heads
    tag = "swinforms.attn." + attn_id(case)
    qkv = fill.hash_tensor((B, H, W, 3 * C), tag + ".qkv", {"hashed": 1.0, "peaked": 4.0, "table": 0.1}[case.kind])
    bias = fill.hash_tensor((3 * C,), tag + ".bias", 0.5)
    table = fill.hash_tensor((169, heads), tag + ".table", 20.0 if case.kind == "table" else 0.5)
    return qkv, bias, table, fill.hash_tensor((B, H, W, C), tag + ".dout", 1.0)


@functools.lru_cache(maxsize=None)
def attn_reference(case):
    qkv, bias, table, dout = attn_data(case)
    return fp64ref.window_attention(qkv, bias, table, case.geom[3], case.geom[4], dout)


ATTN_DEFECTS = ("region label off by one", "bias table indexed transposed", "scale missing", "scale applied twice",
                "padding keys zero", "padding keys left out of d_qkv_bias")


def torch_attention(qkv, bias, table, heads, shift, dout, dtype=torch.float32, defect=None):
    """The torch restatement of the attention core in `dtype` with autograd: {"out", "d_qkv", "d_table", "d_qkv_bias"}.  The partition
    is fp64ref.window_index's (which test_fp64ref_swin_host.py pins to swin_ref.attn_core); the arithmetic is matmul / softmax."""
    q_, b_, t_ = (t.detach().to(dtype).clone().requires_grad_(True) for t in (qkv, bias, table))
    B, H, W, C3 = q_.shape
    C, D = C3 // 3, 32
    Y, X, lab, rel, (sh, sw) = fp64ref.window_index(H, W, shift)
    Ph, Pw = int(Y.max()) + 1, int(X.max()) + 1
    if defect == ATTN_DEFECTS[0]:          # > for >=
        ry, rx = (Y - sh) % Ph, (X - sw) % Pw
        ly = 0 if sh == 0 else (ry > Ph - WIN).long() + (ry > Ph - sh).long()
        lx = 0 if sw == 0 else (rx > Pw - WIN).long() + (rx > Pw - sw).long()
        lab = ly * 3 + lx + torch.zeros_like(Y)
    if defect == ATTN_DEFECTS[1]:          # (dx + 6) * 13 + (dy + 6)
        rel = (rel % 13) * 13 + rel // 13
    scale = {ATTN_DEFECTS[2]: 1.0, ATTN_DEFECTS[3]: 1.0 / D}.get(defect, D ** -0.5)
    full = (torch.zeros(B, Ph, Pw, C3, dtype=dtype) + (0.0 * b_ if defect == ATTN_DEFECTS[4] else b_)).clone()
    full[:, :H, :W] = q_
    nW = Y.shape[0]
    tok = full[:, Y, X].reshape(B, nW, 49, 3, heads, D).permute(3, 0, 1, 4, 2, 5)
    s = scale * (tok[0] @ tok[1].transpose(-1, -2)) + t_[rel].permute(2, 0, 1)
    s = s + ((lab[:, :, None] != lab[:, None, :]).to(dtype) * -100.0)[:, None]
    o = (torch.softmax(s, dim=-1) @ tok[2]).permute(0, 1, 3, 2, 4).reshape(B, nW, 49, C)
    out = torch.zeros(B, Ph, Pw, C, dtype=dtype).index_put((torch.arange(B)[:, None, None], Y[None], X[None]), o)[:, :H, :W]
    dq, db, dt = torch.autograd.grad(out, (q_, b_, t_), dout.to(dtype))
    if defect == ATTN_DEFECTS[5]:
        db = torch.zeros_like(db)
    return {"out": out.detach(), "d_qkv": dq, "d_table": dt, "d_qkv_bias": db}


@functools.lru_cache(maxsize=None)
def attn_e32(case):
    """{output: e_max} of the fp32 torch restatement against fp64 on the case's data."""
    got, ref = torch_attention(*attn_data(case)[:3], case.geom[3], case.geom[4], attn_data(case)[3]), attn_reference(case)
    return {n: fp64ref.errors(got[n], *ref[n])[0] for n in ref}


def attn_limit(case, out):
    """max(bar A, 2 x fp32 torch on the same data): the rule of attn_cases.limit."""
    return max(BAR_A, 2.0 * attn_e32(case)[out])


# ------------------------------------------------------------------------------------------------ the stem
STEM_E = (32, 64, 96, 128, 160, 192, 256, 288, 384, 512)
STEM_SMALL = ((2, 30, 46), (1, 4, 4))          # W % 4 != 0: the scalar patch load; one token
STEM_CAPPED = (((1, 260, 256), 160), ((1, 260, 256), 512), ((1, 728, 728), 32))          # the backward grid at its cap
STEM_CONTENTS = ("plain", "offset", "zero")
StemCase = collections.namedtuple("StemCase", "geom E content")
STEM_CASES = ([StemCase(g, E, c) for E in STEM_E for g in STEM_SMALL for c in STEM_CONTENTS]
              + [StemCase(g, E, c) for g, E in STEM_CAPPED for c in ("plain", "offset")])


def stem_id(case):
    return f"E{case.E}-{case.geom[0]}x{case.geom[1]}x{case.geom[2]}-{case.content}"


@functools.lru_cache(maxsize=None)
def stem_params(E):
    """(w [E, 1, 4, 4], cb, gamma, beta) fp32, swin_sci_ref's fill."""
    return tuple(t.to(torch.float32) for t in S.stem_params(E).values())


@functools.lru_cache(maxsize=None)
def stem_data(case):
    """(x [B, 1, H, W], dy [B, H//4, W//4, E]) fp32: plain uniform in [-1, 1), the same + 300, all zero."""
    B, H, W = case.geom
    tag = f"swinforms.stem.{B}.{H}.{W}"
    x = torch.zeros(B, 1, H, W) if case.content == "zero" else fill.hash_tensor((B, 1, H, W), tag + ".x", 1.0)
    if case.content == "offset":
        x = x + 300.0
    return x, fill.hash_tensor((B, H // 4, W // 4, case.E), tag + f".dy{case.E}", 1.0)


@functools.lru_cache(maxsize=None)
def stem_reference(case):
    x, dy = stem_data(case)
    return fp64ref.patch_embed_ln(x, *stem_params(case.E), EPS, dy)


STEM_DEFECTS = ("mean divided by G 4 Q",)


def torch_stem(x, w, cb, gamma, beta, dy, dtype=torch.float32, defect=None, lanes=None):
    """The torch restatement of the stem in `dtype` with autograd (swin_sci_ref.stem): {"y", "dW", "db", "dgamma", "dbeta"}.
    defect: the mean taken over `lanes` = G 4 Q slots instead of the E channels."""
    ps = [t.detach().to(dtype).clone().requires_grad_(True) for t in (w, cb, gamma, beta)]
    xx = x.to(dtype)
    if defect is None:
        y = S.stem(dict(zip(S.STEM_NAMES, ps)), xx, EPS)
    else:
        c = F.conv2d(xx, ps[0], ps[1], stride=4).permute(0, 2, 3, 1)
        mean = c.sum(dim=-1, keepdim=True) / lanes
        y = (c - mean) / torch.sqrt((c - mean).square().mean(dim=-1, keepdim=True) + EPS) * ps[2] + ps[3]
    g = torch.autograd.grad(y, ps, dy.to(dtype))
    return {"y": y.detach(), "dW": g[0], "db": g[1], "dgamma": g[2], "dbeta": g[3]}


@functools.lru_cache(maxsize=None)
def stem_e32(case):
    x, dy = stem_data(case)
    got, ref = torch_stem(x, *stem_params(case.E), dy), stem_reference(case)
    return {n: fp64ref.errors(got[n], *ref[n])[0] for n in ref}


def stem_limit(case, out):
    return max(BAR_A, 2.0 * stem_e32(case)[out])


# ------------------------------------------------------------------------------------------------ rowscale_add
# (B, n): n = 4; 3 x 700 floats = 525 float4: three workgroups of 256, the last partial; s of each sample
ROWSCALE_CASES = [(4, 4), (3, 700), (4, 1024)]
ROWSCALE_S = (0.0, 1.0, 2.0, -0.5)


@functools.lru_cache(maxsize=None)
def rowscale_data(case):
    """(x, r [B, n], s [B]) fp32; the first four values of x's row 0 hold -0.0, 0.0, 1e-30 and -3.5."""
    B, n = case
    x = fill.hash_tensor((B, n), f"swinforms.rsa.x.{B}.{n}", 1.0)
    x[0, :4] = torch.tensor([-0.0, 0.0, 1e-30, -3.5])
    r = fill.hash_tensor((B, n), f"swinforms.rsa.r.{B}.{n}", 2.0)
    return x, r, torch.tensor([ROWSCALE_S[i % 4] for i in range(B)])


# ------------------------------------------------------------------------------------------------ what the tables reach
def ln_forms_reached():
    return {ln_label(False, C) for _, C in LN_CASES} | {ln_label(True, 4 * c[3]) for c in MERGE_CASES}


def pe_forms_reached():
    return {pe_label(c.E) for c in STEM_CASES}
