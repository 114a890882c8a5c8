"""GPU: the one-launch weight repack.  (1) adm_pack_weight_table on hand-made tables: every destination column on its own (the f32
operands may be absent, the 16-bit images leave as 8-byte stores) against the per-layer kernels, bit for bit, with canary margins
around every destination; (2) the host rule of adm_amd.ops: repack_all() refreshes the f32 operands that were read since the
previous repack and no others, a stale one is refreshed by its next read, a steady loop does not rebuild the table; (3) the affine
group's transposed operand without the in-place identity of its forward operand."""
import pytest
import torch

from oracle import fill

pytestmark = pytest.mark.gpu

LAYERS = ((33, 47, 9, 0),      # ragged both ways, 2 x 2 tiles
          (96, 64, 9, 0),      # plain 3x3
          (192, 64, 1, 1),     # qkv row permutation
          (40, 24, 1, 0))      # ragged 1x1
IMAGES = {9: ("w2f6", "w2b6", "w2fh", "w2bh"), 1: ("g6f", "g6b", "g6fh", "g6bh")}      # the 16-bit images, per taps
F32 = {9: ("fwd", "bwd", "wf", "wb", "w2f", "w2b"), 1: ("fwd", "bwd")}
MARGIN = 64                    # canary elements on either side of a destination (a multiple of 8 bytes for every dtype)
CANARY = 0x5A5B


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).reshape(-1)


def _reference(w, co, ci, taps, qkv, scale, flag):
    """Every operand of one layer from the per-layer kernels: name -> tensor."""
    from adm_amd.hip import call, ptr
    gpu, ks = w.device, 3 if taps == 9 else 1
    cop, cip = (co + 31) // 32 * 32, (ci + 31) // 32 * 32
    new = lambda shape, dtype=torch.float32: torch.empty(shape, device=gpu, dtype=dtype)
    r = {"fwd": new((cop, taps * cip)), "bwd": new((cip, taps * cop))}
    call("adm_pack_weight", ptr(w), ptr(r["fwd"]), ptr(r["bwd"]), co, ci, ks, cop, cip, qkv)
    if taps == 9:
        r["wf"], r["wb"] = new((4, cop, 3, cip)), new((4, cip, 3, cop))
        call("adm_pack_weight_wino", ptr(w), ptr(r["wf"]), ptr(r["wb"]), co, ci, cop, cip)
        r["w2f"], r["w2b"] = new((16, cop, cip)), new((16, cip, cop))
        call("adm_pack_weight_wino2d", ptr(w), ptr(r["w2f"]), ptr(r["w2b"]), co, ci, cop, cip)
        for d in "fb":
            src = r["w2" + d]
            rows, cols = src.shape[1], src.shape[2]
            r[f"w2{d}6"] = new((16, 3, rows, cols), torch.bfloat16)
            call("adm_split3_bf16", ptr(src), ptr(r[f"w2{d}6"]), rows, cols)
            r[f"w2{d}h"] = new((16, 2, rows, cols), torch.float16)
            call("adm_split2_f16", ptr(src), ptr(r[f"w2{d}h"]), rows, cols, scale, ptr(flag))
    else:
        for d, src in (("f", r["fwd"]), ("b", r["bwd"])):
            rows, cols = src.shape
            r[f"g6{d}"] = new((3, rows, cols), torch.bfloat16)
            call("adm_split3_rows", ptr(src), ptr(r[f"g6{d}"]), rows, cols, cols)
            r[f"g6{d}h"] = new((2, rows, cols), torch.float16)
            call("adm_split2_rows_f16", ptr(src), ptr(r[f"g6{d}h"]), rows, cols, cols, scale, ptr(flag))
    return r


def test_table_kernel_writes_each_destination_on_its_own():
    gpu = _gpu()
    from adm_amd import ops
    from adm_amd.hip import call, ptr
    scale = ops.H3_WSCALE
    flags = torch.zeros(4, dtype=torch.int32, device=gpu)      # 0: reference kernels, 1: hash-filled rows, 2 / 3: the two rows of 40.0
    flag_ptr = lambda i: flags.data_ptr() + 4 * i
    col = dict(ops._PACK_IMAGES, fwd=ops.PT_FWD, bwd=ops.PT_BWD)
    rows, checks, keep, tiles = [], [], [], 0

    def add_row(w, co, ci, taps, qkv, names, ref, flag):
        nonlocal tiles
        row = [0] * ops.PACK_TABLE_COLS
        cop, cip = ops.ceil32(co), ops.ceil32(ci)
        row[ops.PT_SRC], row[ops.PT_CO], row[ops.PT_CI], row[ops.PT_TAPS] = w.data_ptr(), co, ci, taps
        row[ops.PT_CO_PAD], row[ops.PT_CI_PAD], row[ops.PT_QKV], row[ops.PT_TILE_BEGIN] = cop, cip, qkv, tiles
        row[ops.PT_H3_SCALE] = ops._H3_WSCALE_BITS
        if any(n in ops._H3_IMAGES for n in names):
            row[ops.PT_H3_FLAG] = flag
        for n in names:
            exp = _bits(ref[n]) if ref is not None else None
            numel = exp.numel() if exp is not None else (16 if taps == 9 else 1) * 2 * cop * cip
            buf = torch.full((numel + 2 * MARGIN,), CANARY, device=gpu, dtype=exp.dtype if exp is not None else torch.int16)
            row[col[n]] = buf.data_ptr() + MARGIN * buf.element_size()
            checks.append(((co, ci, taps, qkv, tuple(names), n), buf, exp))
        rows.append(row)
        tiles += (cop // 32) * (cip // 32)

    for co, ci, taps, qkv in LAYERS:
        ks = 3 if taps == 9 else 1
        w = fill.hash_tensor((co, ci, ks, ks), f"rp{co}.{ci}.{taps}", 0.3).to(gpu)
        keep.append(w)
        ref = _reference(w, co, ci, taps, qkv, scale, flags[0:1])
        imgs, f32 = IMAGES[taps], F32[taps]
        variants = [f32 + imgs, f32[2:] + imgs, ("fwd",), ("bwd",)] + [(n,) for n in imgs]
        for names in variants:
            add_row(w, co, ci, taps, qkv, names, ref, flag_ptr(1))
    for i, (taps, name) in enumerate(((9, "w2fh"), (1, "g6fh"))):      # 40 * 2^11 leaves the fp16 range
        big = torch.full((32, 32, 3 if taps == 9 else 1, 3 if taps == 9 else 1), 40.0, device=gpu)
        keep.append(big)
        add_row(big, 32, 32, taps, 0, (name,), None, flag_ptr(2 + i))
    table = torch.tensor(rows, dtype=torch.int64).to(gpu)
    call("adm_pack_weight_table", ptr(table), len(rows), tiles)
    torch.cuda.synchronize()
    assert flags.tolist() == [0, 0, 1, 1], flags.tolist()
    for what, buf, exp in checks:
        assert bool((buf[:MARGIN] == CANARY).all()) and bool((buf[-MARGIN:] == CANARY).all()), ("canary", what)
        if exp is not None:
            assert torch.equal(buf[MARGIN:-MARGIN], exp), what


def _nhwc(t, gpu):
    return t.permute(0, 2, 3, 1).contiguous().to(gpu)


def test_repack_all_refreshes_only_the_f32_operands_that_were_read(monkeypatch):
    gpu = _gpu()
    from adm_amd import hip, ops
    for name, value in (("WINOGRAD", True), ("WINOGRAD2D", True), ("BF16X6", True), ("FP16X3", True), ("COMPUTE", "f32"), ("WINO_MIN_M", 2048)):
        monkeypatch.setattr(ops, name, value)                # the default selection, whatever the environment says
    monkeypatch.setattr(ops, "_pack_registry", {})           # the table of this test holds its own layers only ...
    monkeypatch.setattr(ops, "_pack_table", None)
    monkeypatch.setattr(ops, "_h3_flag", None)               # ... and raises a flag of its own
    monkeypatch.setattr(ops, "PROFILE", [])
    calls = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    xb = _nhwc(fill.hash_tensor((2, 64, 32, 32), "rhx", 1.0), gpu)       # enough pixels for the split kernels
    xs = _nhwc(fill.hash_tensor((1, 64, 8, 8), "rhs", 1.0), gpu)                 # 64 pixels: the direct kernel
    am = ops.amax_vector(xb)
    w1 = torch.nn.Parameter(fill.hash_tensor((96, 64, 3, 3), "rhw1", 0.05).to(gpu))
    w2 = torch.nn.Parameter(fill.hash_tensor((64, 64, 3, 3), "rhw2", 0.05).to(gpu))

    def step():
        with torch.no_grad():
            ops.conv2d(xb, w1, None, amax=am)                 # the fp16 format: reads the image w2fh only
        x = xs.clone().requires_grad_(True)
        ops.conv2d(x, w2, None).sum().backward()              # direct kernels: reads fwd and bwd
        with torch.no_grad():
            for w in (w1, w2):
                w.data.mul_(1.25).add_(0.01)                  # in place, as the optimiser kernel does
        ops.repack_all()

    step()
    kinds = [k[0] for k in ops.PROFILE]
    assert kinds.count("wino2h3") == 1 and kinds.count("igemm") == 2, kinds
    pk1, pk2 = w1._adm_packed, w2._adm_packed
    assert pk1.w2fh is not None
    table = ops._pack_table[0].cpu()
    by_src = {int(r[ops.PT_SRC]): r for r in table}
    r1, r2 = by_src[w1.data_ptr()], by_src[w2.data_ptr()]
    assert int(r1[ops.PT_FWD]) == 0 and int(r1[ops.PT_BWD]) == 0 and int(r1[ops.PT_W2FH]) == pk1.w2fh.data_ptr()
    assert int(r2[ops.PT_FWD]) == pk2._fwd.data_ptr() and int(r2[ops.PT_BWD]) == pk2._bwd.data_ptr()
    builds, refreshes = ops.pack_table_builds, ops.operand_refreshes
    del calls[:]
    step()                                                    # the same reads again: same table, no per-layer launch
    assert ops.pack_table_builds == builds and ops.operand_refreshes == refreshes
    assert "adm_pack_weight" not in calls and calls.count("adm_pack_weight_table") == 1, calls
    assert w1._adm_packed is pk1 and w2._adm_packed is pk2
    # the direct-kernel layer follows the table launch
    f, b = torch.empty_like(pk2._fwd), torch.empty_like(pk2._bwd)
    hip.call("adm_pack_weight", w2.data_ptr(), f.data_ptr(), b.data_ptr(), 64, 64, 3, 64, 64, 0)
    assert torch.equal(f, pk2._fwd) and torch.equal(b, pk2._bwd)
    # the first layer's f32 operands are two repacks behind; driven through the direct kernel it reads current ones
    fresh = w1.detach().clone()                               # (no parameter: it stays out of the repack table)
    with torch.no_grad():
        y_old, y_new = ops.conv2d(xs, w1, None), ops.conv2d(xs, fresh, None)
    assert calls.count("adm_pack_weight") == 2                # one refresh of w1's fwd, one pack of the fresh parameter
    assert ops.operand_refreshes == refreshes + 1
    assert torch.equal(y_old, y_new)
    f, b = torch.empty_like(pk1._fwd), torch.empty_like(pk1._bwd)
    hip.call("adm_pack_weight", w1.data_ptr(), f.data_ptr(), b.data_ptr(), 96, 64, 3, 96, 64, 0)
    assert torch.equal(pk1.fwd, f) and not torch.equal(pk1._bwd, b)      # bwd was not asked for: still stale ...
    assert torch.equal(pk1.bwd, b)                                       # ... until it is read
    # what was read is back in the table of the next repack
    ops.repack_all()
    assert ops.pack_table_builds == builds + 1
    r1 = {int(r[ops.PT_SRC]): r for r in ops._pack_table[0].cpu()}[w1.data_ptr()]
    assert int(r1[ops.PT_FWD]) == pk1._fwd.data_ptr() and int(r1[ops.PT_BWD]) == pk1._bwd.data_ptr()


def test_affine_group_transposed_without_the_identity(monkeypatch):
    gpu = _gpu()
    from adm_amd import ops
    monkeypatch.setattr(ops, "_pack_registry", {})
    monkeypatch.setattr(ops, "_pack_table", None)
    lins = [torch.nn.Linear(64, n).to(gpu) for n in (64, 128, 96)]
    grp = ops.AffineGroup(lins)
    grp.operands()
    grp.transposed()
    for _ in range(2):                                        # the second round runs on the cached tables
        with torch.no_grad():
            for l in lins:
                l.weight.data.mul_(0.5).add_(0.125)              # in place, same version: as the optimiser kernel does
        ops.repack_all()
        wcat, _ = grp.operands()
        wt = grp.transposed()
        assert int(grp.t_table[0, ops.PT_FWD]) == 0 and int(grp.t_table[0, ops.PT_BWD]) == wt.data_ptr()
        assert torch.equal(wt, wcat.t())
        assert torch.equal(wcat, torch.cat([l.weight.detach() for l in lins]))      # = adm_pack_weight of a [out][in] matrix
        row = {int(r[ops.PT_SRC]): r for r in ops._pack_table[0].cpu()}[lins[1].weight.data_ptr()]
        assert int(row[ops.PT_FWD]) == wcat[64:192].data_ptr() and int(row[ops.PT_BWD]) == 0      # the per-layer bwd has no reader
