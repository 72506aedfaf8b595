#!/usr/bin/env python3
"""Cost of the opt-in multi-level transform against the one-level codec, one library build.

On a bench_workloads shape (default C2: 1024 x 64^3 fp64), device buffers, the
context's own stream, host clock around call + wc_synchronize, alternating:
  forward
    stage_emit_keep   wc_forward_stage(NULL) + wc_forward_emit at the workload's keep: the same
                      dense staging with one level (a)
    levels{2,3,4}_keep  wc_forward_levels with the keep rule (b)
    levels2_thresh    wc_forward_levels with an explicit threshold: no key pass
    forward_default   wc_forward (sparse staging), for scale
  inverse, of the payloads each forward wrote
    inverse_levels{2,3,4}   wc_inverse_levels
    inverse_dense     wc_inverse with WC_OPT_INVERSE_ROWS = 0 (the same dense decode, one level)
    inverse_default   wc_inverse (row-indexed)
Medians of --steps calls each after --warmup, then one profiled pass per leg for
the stage times (WC_STAGE_LEVELS among them); per leg also the kept pairs, the
payload bytes and the RMSE of its round trip (wc_rmse, root mean square over units).

Estimate from bytes, written before the first run (N = the batch's cells, fp32
coefficients; rates of profiles/r06/experiments/gpu_bw_mix.txt, plain accesses):
  a level pass l moves N / 8^(l-1) coefficients four times: read from the
    coefficient scratch and written to the side scratch, then read there and
    written back: 16 B per coefficient of the sub-box, at the 1:1 mix's 5.06 TB/s;
  the key pass of the keep rule reads the final array once: 4 B per coefficient
    at the read-only 5.87 TB/s.
  C2 (N = 268.4 M): level 2 0.537 GB = 0.106 ms, levels 2-3 0.604 GB = 0.119 ms,
  levels 2-4 0.612 GB = 0.121 ms; key pass 1.074 GB = 0.183 ms.  So (b) - (a):
  0.289 / 0.302 / 0.304 ms at L = 2 / 3 / 4, and 0.106 ms with an explicit threshold.
The inverse adds the level passes only (no key pass) to the dense decode.

    python tools/bench_levels.py --steps 30 --warmup 5 --out profiles/r08/levels.json
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

MIX_TB_S = 5.06   # 1:1 reads and writes, plain
READ_TB_S = 5.87  # read only, plain


def estimate_ms(ncells: int, levels: int, key: bool) -> float:
    gb = sum(16.0 * ncells / 8 ** (l - 1) for l in range(2, levels + 1)) / 1e9
    return gb / MIX_TB_S + (4.0 * ncells / 1e9 / READ_TB_S if key else 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--thresh", type=float, default=0.35, help="the explicit threshold of levels2_thresh")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps >= 20")

    import numpy as np
    import torch
    import wcamd
    import bench_workloads as bw
    capi = wcamd.capi

    if not torch.cuda.is_available():
        raise SystemExit("bench_levels.py needs a HIP device")
    dev = torch.device("cuda", 0)
    wl = bw.WORKLOADS[args.workload]
    units_py = wl["units"]()
    cells, offsets, extent = bw.synth_cells(torch, dev, units_py, wl["dtype"])
    units, n, _ = bw.units_array(capi, units_py, offsets)
    dtype = capi.WC_F64 if wl["dtype"] == "f64" else capi.WC_F32
    keep = float(np.float32(wl["keep"]))
    ncells = sum(u.cells for u in units_py)
    lv = {L: [capi.levels_for(units[i].nx, units[i].ny, units[i].nz, L) for i in range(n)] for L in (2, 3, 4)}
    cap = capi.payload_bound(units, n)
    pays = {k: torch.empty(cap, dtype=torch.uint8, device=dev) for k in ("one", "multi")}
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    kept = torch.zeros(n, dtype=torch.int32, device=dev)
    regen = torch.empty(max(extent, 1), dtype=torch.float32, device=dev)
    rmse = torch.zeros(n, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx = capi.Context(0)

    def outs(which):
        return pays[which].data_ptr(), cap, off.data_ptr(), kept.data_ptr()

    def stage_emit():
        ctx.forward_stage(cells.data_ptr(), dtype, units, n, None)
        ctx.forward_emit(units, n, keep, None, *outs("one"))

    def fwd_levels(L, thresh=None):
        return lambda: ctx.forward_levels(cells.data_ptr(), dtype, units, n, lv[L], keep, thresh, *outs("multi"))

    fwd = {"stage_emit_keep": stage_emit, "levels2_keep": fwd_levels(2), "levels3_keep": fwd_levels(3),
           "levels4_keep": fwd_levels(4), "levels2_thresh": fwd_levels(2, args.thresh),
           "forward_default": lambda: ctx.forward(cells.data_ptr(), dtype, units, n, keep, *outs("one"))}

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def profiled(fn):
        ctx.profile_enable(True)
        fn()
        ctx.synchronize()
        st = {k: round(v[0], 4) for k, v in ctx.profile_read().items()}
        ctx.profile_enable(False)
        return st

    times = {k: [] for k in fwd}
    for step in range(args.warmup + args.steps):
        for name, fn in fwd.items():  # alternating: drift hits every variant alike
            dt = timed(fn)
            if step >= args.warmup:
                times[name].append(dt)

    def inv_levels(L):
        return lambda: ctx.inverse_levels(pays["multi"].data_ptr(), off.data_ptr(), units, n, lv[L], regen.data_ptr())

    def inv_one():
        ctx.inverse(pays["one"].data_ptr(), off.data_ptr(), units, n, regen.data_ptr())

    def inv_dense():
        ctx.set_option(capi.WC_OPT_INVERSE_ROWS, 0)
        try:
            inv_one()
        finally:
            ctx.set_option(capi.WC_OPT_INVERSE_ROWS, 1)

    # per forward leg: kept pairs, payload bytes, the round trip's RMSE and stage times
    legs, stages = {}, {}
    inv_of = {"stage_emit_keep": inv_one, "forward_default": inv_one, "levels2_keep": inv_levels(2),
              "levels3_keep": inv_levels(3), "levels4_keep": inv_levels(4), "levels2_thresh": inv_levels(2)}
    for name, fn in fwd.items():
        stages[name] = profiled(fn)
        inv_of[name]()
        ctx.rmse(cells.data_ptr(), dtype, regen.data_ptr(), units, n, rmse.data_ptr())
        ctx.synchronize()
        k = int(kept.sum().item())
        legs[name] = {"kept_pairs": k, "payload_bytes": 20 * n + 8 * k,
                      "rmse": math.sqrt(float((rmse * rmse).mean().item()))}

    ctx.forward(cells.data_ptr(), dtype, units, n, keep, *outs("one"))
    ctx.synchronize()
    itimes = {}
    for L in (2, 3, 4):
        fwd_levels(L)()
        ctx.synchronize()
        inv = {f"inverse_levels{L}": inv_levels(L), "inverse_dense": inv_dense, "inverse_default": inv_one}
        for step in range(args.warmup + args.steps):
            for name, fn in inv.items():
                dt = timed(fn)
                if step >= args.warmup:
                    itimes.setdefault(name, []).append(dt)
        stages[f"inverse_levels{L}"] = profiled(inv[f"inverse_levels{L}"])
    stages["inverse_dense"] = profiled(inv_dense)
    stages["inverse_default"] = profiled(inv_one)
    times.update(itimes)

    med = {k: statistics.median(v) for k, v in times.items()}
    res = {
        "bench": "levels", "workload": args.workload, "units": n, "cells": ncells, "dtype": wl["dtype"],
        "steps": args.steps, "warmup": args.warmup, "keep": keep, "thresh": args.thresh,
        "ms_median": {k: round(v, 4) for k, v in med.items()},
        "ms_min": {k: round(min(v), 4) for k, v in times.items()},
        "ms_p90": {k: round(sorted(v)[int(0.9 * (len(v) - 1))], 4) for k, v in times.items()},
        "legs": legs, "stage_ms": stages,
        "levels_minus_stage_emit_ms": {k: round(med[k] - med["stage_emit_keep"], 4)
                                       for k in ("levels2_keep", "levels3_keep", "levels4_keep", "levels2_thresh")},
        "estimate_ms": {"levels2_keep": round(estimate_ms(ncells, 2, True), 4),
                        "levels3_keep": round(estimate_ms(ncells, 3, True), 4),
                        "levels4_keep": round(estimate_ms(ncells, 4, True), 4),
                        "levels2_thresh": round(estimate_ms(ncells, 2, False), 4)},
        "inverse_levels_minus_dense_ms": {f"L{L}": round(med[f"inverse_levels{L}"] - med["inverse_dense"], 4)
                                          for L in (2, 3, 4)},
        "inverse_estimate_ms": {f"L{L}": round(estimate_ms(ncells, L, False), 4) for L in (2, 3, 4)},
        "mix_tb_s_assumed": MIX_TB_S, "read_tb_s_assumed": READ_TB_S,
        "device": torch.cuda.get_device_name(0), "library": capi.load_library().wc_version().decode(),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
