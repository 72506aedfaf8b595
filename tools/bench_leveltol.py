#!/usr/bin/env python3
"""Cost of the RMSE tolerance on the multi-level transform, one library build.

On a bench_workloads shape (default C2: 1024 x 64^3 fp64), device buffers, the
context's own stream, host clock around call + wc_synchronize, alternating, for
L = 1..4 (each unit at wc_levels_for(dims, L)):
    leveltol_L        wc_forward_levels_tol, every unit's tolerance = --frac times its RMS
    levels_thresh_L   wc_forward_levels with an explicit threshold: the same dense
                      staging, level passes and emit with one threshold (a)
and once
    forward_tol       wc_forward_tol at the same tolerances (b)
Medians of --steps calls each after --warmup, then one profiled pass per leg for
the stage times (WC_STAGE_TOL: the per-level bins, the pick and the mask pass);
per leg also the kept pairs, the payload bytes and the actual RMSE of its round
trip (wc_inverse_levels + wc_rmse: root mean square over units, and the largest
ratio of a unit's RMSE to its tolerance).

Estimate from bytes, written before the first run (N = the batch's cells, fp32
coefficients; rates of profiles/r06/experiments/gpu_bw_mix.txt, plain accesses):
over (a) the bins read the final array once, 4 B per coefficient at the read-only
5.87 TB/s, and the mask pass reads it again and writes it back, 8 B per
coefficient at the 1:1 mix's 5.06 TB/s.  C2 (N = 268.4 M): 1.074 GB = 0.183 ms
plus 2.147 GB = 0.424 ms, 0.607 ms in all.  The mask pass stores only the 16-B
groups it changed, so it moves between 4 and 8 B per coefficient: 0.183 ms to
0.424 ms, and the whole stage 0.366 ms to 0.607 ms.

    python tools/bench_leveltol.py --steps 30 --warmup 5 --out profiles/r11/leveltol.json
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


def estimate_ms(ncells: int):
    bins = 4.0 * ncells / 1e9 / READ_TB_S
    return {"bins": round(bins, 4), "mask_all_stored": round(8.0 * ncells / 1e9 / MIX_TB_S, 4),
            "mask_nothing_stored": round(bins, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frac", type=float, default=0.01, help="each unit's tolerance as a fraction of its RMS")
    ap.add_argument("--thresh", type=float, default=0.35, help="the explicit threshold of the levels_thresh legs")
    ap.add_argument("--levels", default="1,2,3,4", help="the L of the leveltol / levels_thresh legs (a kernel trace of one L)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    Ls = tuple(int(x) for x in args.levels.split(","))
    if args.steps < 20:
        ap.error("--steps >= 20")

    import numpy as np
    import torch
    import wcamd
    import bench_workloads as bw
    capi = wcamd.capi

    if not torch.cuda.is_available():
        raise SystemExit("bench_leveltol.py needs a HIP device")
    dev = torch.device("cuda", 0)
    wl = bw.WORKLOADS[args.workload]
    units_py = wl["units"]()
    cells, offsets, extent = bw.synth_cells(torch, dev, units_py, wl["dtype"])
    units, n, _ = bw.units_array(capi, units_py, offsets)
    dtype = capi.WC_F64 if wl["dtype"] == "f64" else capi.WC_F32
    ncells = sum(u.cells for u in units_py)
    sizes = [units[i].nx * units[i].ny * units[i].nz for i in range(n)]
    rms = np.array([float(cells[units[i].cell_offset:units[i].cell_offset + sizes[i]].double().pow(2).mean().sqrt().item())
                    if sizes[i] else 0.0 for i in range(n)])
    tol = args.frac * rms
    tol_d = torch.from_numpy(tol).to(dev)
    lv = {L: [capi.levels_for(units[i].nx, units[i].ny, units[i].nz, L) for i in range(n)] for L in (1, 2, 3, 4)}
    cap = capi.payload_bound(units, n)
    pay = torch.empty(cap, dtype=torch.uint8, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    kept = torch.zeros(n, dtype=torch.int32, device=dev)
    thresh = torch.zeros(n * capi.WC_MAX_LEVELS, dtype=torch.float32, device=dev)
    bound = torch.zeros(n, dtype=torch.float64, device=dev)
    regen = torch.empty(max(extent, 1), dtype=torch.float32, device=dev)
    rmse = torch.zeros(n, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx = capi.Context(0)
    outs = (pay.data_ptr(), cap, off.data_ptr(), kept.data_ptr())

    def leveltol(L):
        return lambda: ctx.forward_levels_tol(cells.data_ptr(), dtype, units, n, lv[L], tol, *outs, thresh.data_ptr(),
                                              bound.data_ptr())

    def levels_thresh(L):
        return lambda: ctx.forward_levels(cells.data_ptr(), dtype, units, n, lv[L], 0.0, args.thresh, *outs)

    fwd = {}
    for L in Ls:
        fwd[f"leveltol_L{L}"] = leveltol(L)
        fwd[f"levels_thresh_L{L}"] = levels_thresh(L)
    fwd["forward_tol"] = lambda: ctx.forward_tol(cells.data_ptr(), dtype, units, n, tol, *outs, thresh.data_ptr(),
                                                 bound.data_ptr())
    level_of = {k: int(k[-1]) if k[-1].isdigit() else 1 for k in fwd}

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    times = {k: [] for k in fwd}
    for step in range(args.warmup + args.steps):
        for name, fn in fwd.items():  # alternating: drift hits every variant alike
            dt = timed(fn)
            if step >= args.warmup:
                times[name].append(dt)

    legs, stages = {}, {}
    for name, fn in fwd.items():
        ctx.profile_enable(True)
        fn()
        ctx.synchronize()
        st = {k: round(v[0], 4) for k, v in ctx.profile_read().items()}
        ctx.profile_enable(False)
        stages[name] = st
        ctx.inverse_levels(pay.data_ptr(), off.data_ptr(), units, n, lv[level_of[name]], regen.data_ptr())
        ctx.rmse(cells.data_ptr(), dtype, regen.data_ptr(), units, n, rmse.data_ptr())
        ctx.synchronize()
        k = int(kept.sum().item())
        legs[name] = {"kept_pairs": k, "payload_bytes": 20 * n + 8 * k,
                      "rmse": math.sqrt(float((rmse * rmse).mean().item())),
                      "tol_share_of_stages": round(st.get("tol", 0.0) / max(sum(st.values()), 1e-9), 4)}
        if not name.startswith("levels_thresh"):
            legs[name]["max_rmse_over_tol"] = float((rmse / tol_d).max().item())
            legs[name]["max_bound_over_tol"] = float((bound / tol_d).max().item())

    med = {k: statistics.median(v) for k, v in times.items()}
    res = {
        "bench": "leveltol", "workload": args.workload, "units": n, "cells": ncells, "dtype": wl["dtype"],
        "steps": args.steps, "warmup": args.warmup, "frac": args.frac, "thresh": args.thresh,
        "tol_rms": math.sqrt(float(np.mean(tol * tol))),
        "ms_median": {k: round(v, 4) for k, v in med.items()},
        "ms_min": {k: round(min(v), 4) for k, v in times.items()},
        "ms_p90": {k: round(sorted(v)[int(0.9 * (len(v) - 1))], 4) for k, v in times.items()},
        "legs": legs, "stage_ms": stages,
        "leveltol_minus_levels_thresh_ms": {f"L{L}": round(med[f"leveltol_L{L}"] - med[f"levels_thresh_L{L}"], 4)
                                            for L in Ls},
        "leveltol_L1_minus_forward_tol_ms": round(med["leveltol_L1"] - med["forward_tol"], 4) if 1 in Ls else None,
        "estimate_ms": estimate_ms(ncells),
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
