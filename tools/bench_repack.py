"""Micro-benchmark of adm_pack_weight_table (C ABI) on the repack table of the benchmark model.

Four training steps of bench.py's model build the table adm_amd.ops.repack_all() issues; its host rows are then launched as
  today    every row with both f32 operands (fwd, bwd) and its images: what every repack wrote before the f32 operands went on demand
  read     the f32 columns of operands nobody read since the previous repack zeroed: what repack_all() issues now
  images   every f32 column zeroed (the floor: images alone)
and, for the affine group's one-row table, with and without the forward image onto itself.  --parent-lib PATH launches `today` (the
only table a library from before the optional columns can take: it writes fwd and bwd unconditionally) through that library too, on
the same pointers, which compares the store paths of the 16-bit images.  Bytes = source read + every destination written.

    python3 tools/bench_repack.py [--parent-lib /path/to/parent/libadm_hip.so] [--iters 50] [--json OUT]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def row_bytes(ops, row):
    co, ci, taps, cop, cip = (row[c] for c in (ops.PT_CO, ops.PT_CI, ops.PT_TAPS, ops.PT_CO_PAD, ops.PT_CI_PAD))
    per = {ops.PT_FWD: 4 * taps, ops.PT_BWD: 4 * taps, ops.PT_WF: 48, ops.PT_WB: 48, ops.PT_W2F: 64, ops.PT_W2B: 64,
           ops.PT_W2F6: 96, ops.PT_W2B6: 96, ops.PT_W2FH: 64, ops.PT_W2BH: 64, ops.PT_G6F: 6, ops.PT_G6B: 6, ops.PT_G6FH: 4, ops.PT_G6BH: 4}
    return 4 * co * ci * taps + sum(b * cop * cip for c, b in per.items() if row[c])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import bench
    from adm_amd import hip, ops
    from adm_amd.optim import FlatParams, FusedAdamWEMA
    dev = torch.device("cuda", 0)
    dpm = bench.build_model(dev)
    dpm.train()
    flat = FlatParams(dpm)
    opt = FusedAdamWEMA(flat, lr=1e-4, weight_decay=1e-4, max_norm=1.0, ema=True)
    batch = {"image": torch.rand(128, 3, 32, 32, device=dev) * 2 - 1}
    counters = []                                         # (table builds, per-layer operand refreshes) after each step
    for _ in range(4):
        flat.zero_grad()
        dpm.training_step(batch)[0].backward()
        opt.step()
        counters.append((ops.pack_table_builds, ops.operand_refreshes))
    torch.cuda.synchronize()
    _, ents, tiles, rows, read = ops._pack_table
    zero = lambda row, m: row[:ops.PT_FWD] + [row[ops.PT_FWD] * (m & 1), row[ops.PT_BWD] * (m >> 1)] + row[ops.PT_BWD + 1:]
    tables = {"today": (rows, tiles), "read": ([zero(r, m) for r, m in zip(rows, read)], tiles),
              "images": ([zero(r, 0) for r in rows], tiles)}
    from adm_amd.unet import dhariwal
    for grp, _blocks in list(dhariwal._AFFINE_GROUPS.values()):
        if grp.t_table is not None:
            r = grp.t_table[0].tolist()
            tables["affine_t (fwd = 0)"] = ([r], (grp.total // 32) * (grp.K // 32))
            tables["affine_t (fwd onto itself)"] = ([r[:ops.PT_FWD] + [r[ops.PT_SRC]] + r[ops.PT_FWD + 1:]], (grp.total // 32) * (grp.K // 32))
    libs = {"head": hip.lib()}
    if args.parent_lib:
        libs["parent"] = ctypes.CDLL(args.parent_lib)
        libs["parent"].adm_pack_weight_table.argtypes = libs["head"].adm_pack_weight_table.argtypes
    params = sum(r[ops.PT_CO] * r[ops.PT_CI] * r[ops.PT_TAPS] for r in rows)
    out = {"layers": len(rows), "parameters": params, "tiles": tiles, "f32 operands in the read set": sum(bin(m).count("1") for m in read),
           "of": 2 * len(rows), "table builds / operand refreshes after each of four steps": counters, "results": []}
    print(json.dumps({k: v for k, v in out.items() if k != "results"}), flush=True)
    for lname, lib in libs.items():
        for tname, (trows, ttiles) in tables.items():
            if lname == "parent" and not (tname == "today" or "itself" in tname):
                continue                                  # a 0 in PT_FWD / PT_BWD is not a table for that library
            table = torch.tensor(trows, dtype=torch.int64).to(dev)
            nbytes = sum(row_bytes(ops, r) for r in trows)
            launch = lambda: lib.adm_pack_weight_table(hip.ptr(table), len(trows), ttiles, hip.stream())
            times = []
            for rep in range(2):
                for _ in range(5):
                    assert launch() == 0
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.iters):
                    launch()
                b.record()
                torch.cuda.synchronize()
                times.append(a.elapsed_time(b) / args.iters)
            res = {"lib": lname, "table": tname, "GB": round(nbytes / 1e9, 4), "ms": [round(t, 4) for t in times],
                   "TB/s": [round(nbytes / t / 1e9, 3) for t in times]}
            out["results"].append(res)
            print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
