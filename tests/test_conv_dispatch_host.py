"""CPU-only: which kernels a conv launches, with which arguments and in which order, is pinned against a recorded trace.

The host path of ops._Conv (and of the strided convs of ops / ops_ae / ops_cond) runs on CPU tensors once the launcher is replaced
by a recorder: the sequence of ``call(name, *args)`` IS its behaviour.  A launch is keyed by its symbol, every int / float argument by
value and every pointer as "p" or 0 (null); the bound look-up and hand-over of gradient tensors (_get_amax / _reg_amax) are recorded
in line, since their order is part of the contract (under ADM_AMAX_CHECK the look-up reads the device).  A case is (forward launches,
backward launches with the end-of-backward flush, whether y carries a bound); packed entries and deferred rows are dropped before each
case, so weight-image builds are part of its trace.  The host queries (adm_*_splitk, adm_*_plan) are pure functions and run in the
real library.

tests/golden/conv_dispatch_trace.json.gz holds the FULL grid.  pytest compares a fixed half of the _Conv grid plus every bf16-storage
and strided case; ``python tests/test_conv_dispatch_host.py`` compares all of it and ``... --write`` records it again -- nothing else
writes the fixture, and it is only ever recorded on a tree whose launches are known to be right.

The ids starting with "side " run with SIDE_WGRAD on: the side stream, its event, torch.cuda.stream() and record_stream() are stubs
that write MARKERS into the same trace, so where the weight-gradient launches sit relative to the side-stream section is pinned too.
"""
import contextlib
import gzip
import itertools
import json
import os
import sys
import zlib

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_dispatch_trace.json.gz")

# (B, H, W, cin, cout, ks, up): both sides of WINO_MIN_M / GEMM_X6_MIN_M, odd and non-power-of-two maps, split-K sized maps, heads and
# stems with 1 or 3 real channels, a qkv-shaped 1x1 (cout % 3 == 0), the Linear shape (H = W = 1) and a fused nearest-x2
GEOMETRIES = ((1, 1, 1, 128, 512, 1, 0), (16, 4, 4, 512, 256, 1, 0), (16, 16, 16, 128, 128, 1, 0), (16, 16, 16, 512, 1, 1, 0),
              (2, 32, 32, 192, 576, 1, 0), (16, 16, 16, 128, 128, 3, 0), (16, 8, 8, 128, 192, 3, 1), (4, 32, 32, 3, 128, 3, 0),
              (4, 32, 32, 128, 3, 3, 0), (8, 5, 6, 64, 64, 3, 0), (8, 7, 6, 64, 64, 3, 0), (2, 4, 4, 64, 96, 3, 0),
              (128, 4, 4, 64, 64, 3, 0),
              (16, 8, 8, 512, 256, 1, 0))       # a 1x1 that reaches GEMM_X6_MIN_M pixels only by batch_invariant(64)'s count
DEFAULTS = dict(WINOGRAD=True, WINO_MIN_M=2048, WINOGRAD2D=True, BF16X6=True, FP16X3=True, H3_WGRAD=True, H3_GEMM=True,
                GEMM_X6_MIN_M=2048, GEMM_WGRAD_X6=True, DETERMINISTIC=False, DEFER_UNPACK=True, COMPUTE="f32", BF16_STORAGE=True,
                SIDE_WGRAD=False, PROFILE=None, AMAX_CHECK=False)
SWITCH_SETS = ({}, {"DETERMINISTIC": True}, {"FP16X3": False}, {"BF16X6": False}, {"WINOGRAD2D": False}, {"WINOGRAD": False},
               {"H3_GEMM": False}, {"H3_WGRAD": False}, {"GEMM_WGRAD_X6": False}, {"DEFER_UNPACK": False}, {"COMPUTE": "bf16"},
               {"COMPUTE": "bf16", "DETERMINISTIC": True}, {"BF16X6": False, "DETERMINISTIC": True})
BF16A_SWITCH_SETS = tuple(dict(s, COMPUTE="bf16") for s in ({}, {"DETERMINISTIC": True}, {"BF16X6": False}, {"GEMM_WGRAD_X6": False},
                                                            {"WINOGRAD2D": False}))
# module state that a case touches: replaced for the duration of a recording, so nothing leaks into other tests
STATE = dict(_pack_registry=dict, _pack_table=None, _rest_ws=dict, _unpack_tables=dict, _gn_tables=dict, _pinned_tables=list,
             _unpack_rows=list, _unpack_keep=list, _unpack_pending=set, _gn_rows=list, _gn_keep=list, _gn_pending=set,
             _amax_pool=None, _amax_next=0, _amax_pool_captured=False, _amax_pool_size=0, _grad_amax=dict, table_uploads=0,
             _unpack_queued=-2, _rows_task=-2, _pack_epoch=0, _SELECT_BATCH=None, _h3_flag=None, _h3_checks=0)

# every symbol that _Conv, _ConvGeneric, _ConvDown and conv2d_strided name in a call(...)
CONV_SYMBOLS = {
    "adm_conv_fwd_wino2d_h3", "adm_gemm_x6_h3", "adm_gemm_x6_amax", "adm_gemm_x6", "adm_conv_fwd_bf16a", "adm_conv_fwd_bf16",
    "adm_conv_fwd_wino2d_x6_up", "adm_conv_fwd_wino2d_x6", "adm_conv_fwd_wino2d", "adm_conv_fwd_wino_up", "adm_conv_fwd_wino",
    "adm_conv_fwd_ws", "adm_conv_fwd", "adm_resample2x",
    "adm_conv_wgrad_x6_bf16a", "adm_gemm_wgrad_x6_bf16a", "adm_conv_wgrad_bf16a", "adm_conv_wgrad_bf16", "adm_conv_wgrad_x6_h3",
    "adm_gemm_wgrad_x6_h3", "adm_gemm_wgrad_x6_ws", "adm_gemm_wgrad_x6", "adm_conv_wgrad_x6_ws", "adm_conv_wgrad_ws",
    "adm_conv_wgrad_x6_up", "adm_conv_wgrad_x6", "adm_conv_wgrad_wino2d", "adm_conv_wgrad_wino_up", "adm_conv_wgrad_wino",
    "adm_conv_wgrad_bias", "adm_unpack_wgrad_wino2d", "adm_unpack_wgrad_splits", "adm_unpack_wgrad", "adm_permute_vec", "adm_colsum",
    "adm_conv_fwd_strided", "adm_pack_weight", "adm_conv_wgrad_strided", "adm_conv_wgrad_strided_ws", "adm_add",
    "adm_pack_weight_tconv", "adm_col2im"}
# ... and what they reach through the packed-weight cache and the end-of-backward table
IMAGE_SYMBOLS = {"adm_pack_weight_wino", "adm_pack_weight_wino2d", "adm_split3_bf16", "adm_split2_f16", "adm_split3_rows",
                 "adm_split2_rows_f16", "adm_f32_to_bf16", "adm_unpack_wgrad_table"}
# the side-stream section of _Conv.backward, in the trace of the "side " cases (record_stream by the role of its tensor)
MARKERS = {"event.record", "side.wait_event", "side.enter", "side.exit", "record_stream", "queue_join"}
# (B, H, W, cin, cout, ks, up, qkv) of the "side " cases: between them the bias routes none / sink / table / permute
SIDE_GEOMETRIES = ((16, 16, 16, 128, 128, 3, 0, 0), (16, 8, 8, 128, 192, 3, 1, 0), (2, 32, 32, 192, 576, 1, 0, 0),
                   (2, 32, 32, 192, 576, 1, 0, 1), (4, 32, 32, 128, 3, 3, 0, 0))
SIDE_SWITCH_SETS = ({}, {"DETERMINISTIC": True}, {"DEFER_UNPACK": False})


def _key(name, args):
    out = [name]
    for a in args:
        if a is None:
            out.append("0")
        elif isinstance(a, (bool, int)):
            out.append(str(int(a)))
        elif isinstance(a, float):
            out.append(repr(a))
        else:                             # ctypes.c_void_p
            out.append("p" if a.value else "0")
    return " ".join(out)


class Recorder:
    """Stubs and switches through one MonkeyPatch; .trace collects the launches of the running case."""

    def __init__(self, mp):
        from adm_amd import hip, ops, ops_ae, ops_cond
        self.mp, self.ops, self.trace, self.dy_bound, self.roles = mp, ops, [], None, {}
        if not os.path.exists(hip.LIB_PATH):
            hip.build()
        record = lambda name, *args: self.trace.append(_key(name, args))
        mp.setattr(hip, "require_cuda", lambda t, what="tensor": None)
        for mod in (ops, ops_ae, ops_cond):      # (each imports `call` by name)
            mp.setattr(mod, "call", record)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)      # raises without a device
        mp.setattr(ops, "_get_amax", lambda t: (self.trace.append("_get_amax"), self.dy_bound)[1])
        mp.setattr(ops, "_reg_amax", lambda t, slot: self.trace.append("_reg_amax " + ("p" if slot is not None else "0")))
        for name, v in STATE.items():
            mp.setattr(ops, name, v() if callable(v) else v)
        # the side-stream section (reached only with SIDE_WGRAD on): every stream / event operation leaves a marker
        mark = self.trace.append

        class Event:
            record = lambda self: mark("event.record")

        class Side:
            wait_event = lambda self, ev: mark("side.wait_event")

        @contextlib.contextmanager
        def on_stream(st):
            mark("side.enter")
            yield
            mark("side.exit")

        side = Side()
        mp.setattr(ops, "_wgrad_stream", lambda: side)
        mp.setattr(torch.cuda, "Event", Event)
        mp.setattr(torch.cuda, "stream", on_stream)
        mp.setattr(torch.Tensor, "record_stream", lambda t, st: mark("record_stream " + self.roles.get(t.data_ptr(), "other")))
        mp.setattr(ops, "_queue_join_at_end_of_backward", lambda: mark("queue_join"))

    def case(self, switches, binv, fn):
        """(forward launches, backward launches, y carries a bound) of fn() -> (y, dy), under DEFAULTS + switches; binv: inside
        batch_invariant(64), the backward too (the data and weight gradients look at the selection batch as well)."""
        ops = self.ops
        with self.mp.context() as m, (ops.batch_invariant(64) if binv else contextlib.nullcontext()):
            for k, v in dict(DEFAULTS, **switches).items():
                m.setattr(ops, k, v)
            ops.invalidate_packed()
            ops.reset_deferred_unpack()
            ops._rest_ws.clear()
            del self.trace[:]
            y, dy = fn()
            fwd = list(self.trace)
            del self.trace[:]
            if y.requires_grad:
                y.backward(dy)
                ops.flush_deferred_unpack()
            return [fwd, list(self.trace), hasattr(y, "_adm_amax")]


def _params(co, ci, ks, bias, direct):
    w, b = torch.empty(co, ci, ks, ks), (torch.empty(co) if bias else None)
    if not direct:
        return w.requires_grad_(), (b.requires_grad_() if bias else None)
    out = []
    for t in (w, b):
        if t is not None:
            t = torch.nn.Parameter(t)
            t.grad, t._adm_direct = torch.zeros_like(t), True
        out.append(t)
    return out


def _conv_case(rec, geom, qkv, bias, res, amax_in, amax_dy, direct, x16=False):
    ops = rec.ops
    B, H, W, ci, co, ks, up = geom
    x = torch.empty(B, H, W, ops.ceil32(ci)).requires_grad_()
    if x16:
        x._adm_bf16 = torch.empty(x.shape, dtype=torch.bfloat16)
    w, b = _params(co, ci, ks, bias, direct)
    r = torch.empty(B, H << up, W << up, ops.ceil32(co)) if res else None
    bound = torch.zeros(ops.AMAX_FLOATS)
    rec.dy_bound = bound if amax_dy else None
    y = ops.conv2d(x, w, b, r, up=bool(up), qkv=bool(qkv), amax=bound if amax_in else None)
    dy = torch.empty_like(y)
    rec.roles = {x.data_ptr(): "x", dy.data_ptr(): "dy"}
    return y, dy


def _strided_case(rec, entry, ks, stride, pads, co, bias, direct):
    from adm_amd import ops_ae, ops_cond
    ops = rec.ops
    x = torch.empty(1, 8, 8, 32).requires_grad_()
    w, b = _params(co, 32, ks, bias, direct)
    if entry == "generic":
        y = ops_cond.conv2d_generic(x, w, b, stride=stride, pad=pads[0])
    elif entry == "down":
        y = ops_ae.conv2d_down(x, w, b, stride=stride, pad_lo=pads[0], pad_hi=pads[1])
    else:
        with torch.no_grad():
            y = ops.conv2d_strided(x, w, b, stride=stride, pad_lo=pads[0], pad_hi=pads[1])
    return y, torch.empty_like(y)


def cases(rec):
    """id -> (switches, inside batch_invariant, thunk) of the whole grid; ids starting with "conv" are the ones pytest thins."""
    out = {}
    sw_name = lambda s: ",".join(f"{k}={v}" for k, v in s.items()) or "default"
    for geom, sw in itertools.product(GEOMETRIES, SWITCH_SETS):
        qkvs = (0, 1) if geom[5] == 1 and geom[4] % 3 == 0 else (0,)
        for qkv, (bias, res), amax_in, amax_dy, direct, binv in itertools.product(qkvs, ((0, 0), (1, 0), (1, 1)), (0, 1), (0, 1), (0, 1),
                                                                                   (0, 1)):
            if binv and (res or qkv):
                continue
            cid = f"conv {'x'.join(map(str, geom))} q{qkv}b{bias}r{res}a{amax_in}g{amax_dy}d{direct}i{binv} {sw_name(sw)}"
            out[cid] = (sw, binv, lambda a=(geom, qkv, bias, res, amax_in, amax_dy, direct): _conv_case(rec, *a))
    # the bf16-stored input (GroupNorm's adm_gn_fwd_bf16out): its values ride on x._adm_bf16
    for geom, sw in itertools.product(GEOMETRIES, BF16A_SWITCH_SETS):
        if rec.ops.ceil32(geom[3]) % 64:
            continue
        qkvs = (0, 1) if geom[5] == 1 and geom[4] % 3 == 0 else (0,)
        for qkv, bias, direct in itertools.product(qkvs, (0, 1), (0, 1)):
            cid = f"bf16a {'x'.join(map(str, geom))} q{qkv}b{bias}d{direct} {sw_name(sw)}"
            out[cid] = (sw, 0, lambda a=(geom, qkv, bias, 0, 0, 0, direct, True): _conv_case(rec, *a))
    strided = (("generic", 4, 2, (1, 1)), ("generic", 7, 1, (3, 3)), ("down", 3, 2, (0, 1)), ("down", 4, 2, (1, 1)),
               ("strided", 3, 2, (0, 1)), ("strided", 4, 2, (1, 1)))
    for (entry, ks, stride, pads), co, bias, direct, det in itertools.product(strided, (32, 3), (0, 1), (0, 1), (0, 1)):
        cid = f"{entry} k{ks}s{stride}p{pads[0]}{pads[1]} co{co} b{bias}d{direct} det{det}"
        out[cid] = ({"DETERMINISTIC": bool(det)}, 0, lambda a=(entry, ks, stride, pads, co, bias, direct): _strided_case(rec, *a))
    # SIDE_WGRAD on; d0 (gradients through autograd) must show no side section
    for geom, sw, bias, bounds, direct in itertools.product(SIDE_GEOMETRIES, SIDE_SWITCH_SETS, (0, 1), (0, 1), (1, 0)):
        if not direct and (sw or not bias or bounds):
            continue
        cid = f"side {'x'.join(map(str, geom[:7]))} q{geom[7]}b{bias}a{bounds}g{bounds}d{direct} {sw_name(sw)}"
        out[cid] = (dict(sw, SIDE_WGRAD=True), 0, lambda a=(geom[:7], geom[7], bias, 0, bounds, bounds, direct): _conv_case(rec, *a))
    return out


def thinned(cid) -> bool:
    return cid.startswith("conv ") and zlib.crc32(cid.encode()) % 2 != 0


def record(mp, keep=lambda cid: True):
    rec = Recorder(mp)
    return {cid: rec.case(sw, binv, fn) for cid, (sw, binv, fn) in cases(rec).items() if keep(cid)}


def load_fixture():
    """The fixture stores each distinct launch once: {"launches": [key, ...], "cases": {id: [[index, ...], [index, ...], bool]}}."""
    with gzip.open(FIXTURE, "rt") as f:
        data = json.load(f)
    names = data["launches"]
    return {cid: [[names[i] for i in fwd], [names[i] for i in bwd], amax] for cid, (fwd, bwd, amax) in data["cases"].items()}


def write_fixture(got):
    index = {}
    enc = lambda launches: [index.setdefault(k, len(index)) for k in launches]
    data = {"cases": {cid: [enc(fwd), enc(bwd), amax] for cid, (fwd, bwd, amax) in got.items()}}
    data["launches"] = list(index)
    with open(FIXTURE, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(json.dumps(data, separators=(",", ":"), sort_keys=True).encode())


def symbols(traces):
    return {k.split(" ", 1)[0] for fwd, bwd, _ in traces.values() for k in fwd + bwd} - {"_get_amax", "_reg_amax"} - MARKERS


def differing(got, want):
    return [cid for cid in got if got[cid] != want.get(cid)]


def test_conv_launches_match_the_recorded_trace(monkeypatch):
    want = load_fixture()
    got = record(monkeypatch, keep=lambda cid: not thinned(cid))
    assert set(got) == {cid for cid in want if not thinned(cid)}
    bad = differing(got, want)
    assert not bad, f"{len(bad)} of {len(got)} cases launch differently, first: {bad[0]}\n got {got[bad[0]]}\nwant {want[bad[0]]}"
    # the thinned grid still reaches everything
    assert symbols(got) == CONV_SYMBOLS | IMAGE_SYMBOLS


def test_fixture_covers_every_conv_symbol():
    want = load_fixture()
    assert symbols(want) == CONV_SYMBOLS | IMAGE_SYMBOLS
    assert sum(cid.startswith("conv ") for cid in want) == 7592
    # a fp16-format data gradient looked its bound up, a 1x1 one handed its own on, a 1x1 forward left one on y
    flat = [k for fwd, bwd, _ in want.values() for k in bwd]
    assert "_get_amax" in flat and "_reg_amax p" in flat and any(amax for _, _, amax in want.values())


def test_fixture_pins_the_side_stream_section():
    want = load_fixture()
    marker = lambda k: k.split(" ", 1)[0] in MARKERS
    wgrad = lambda k: k.startswith(("adm_conv_wgrad", "adm_gemm_wgrad"))
    inside = 0
    for cid, (_, bwd, _) in want.items():
        if not cid.startswith("side "):
            assert not any(map(marker, bwd)), cid
        elif "d0 " in cid:          # nothing can be accumulated directly: everything stays on the main stream
            assert any(map(wgrad, bwd)) and not any(map(marker, bwd)), cid
        elif "side.enter" in bwd:
            inside += any(map(wgrad, bwd[bwd.index("side.enter"):bwd.index("side.exit")]))
    assert inside


if __name__ == "__main__":
    mp = pytest.MonkeyPatch()
    try:
        got = record(mp)
    finally:
        mp.undo()
    if "--write" in sys.argv:
        write_fixture(got)
        print(f"wrote {len(got)} cases, {len(symbols(got))} symbols to {FIXTURE}")
    else:
        want = load_fixture()
        bad = differing(got, want) + [cid for cid in want if cid not in got]
        print(f"{len(got)} cases, {len(bad)} differ from {FIXTURE}")
        for cid in bad[:5]:
            print(cid, "\n got", got.get(cid), "\nwant", want.get(cid))
        sys.exit(1 if bad else 0)
