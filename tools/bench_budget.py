#!/usr/bin/env python3
"""Cost of the size-budget mode (exact per-unit top-K), one library build.

On a bench_workloads shape (default C2: 1024 x 64^3 fp64), device buffers, the
context's own stream, host clock around call + wc_synchronize, alternating, for
L = 1..4 (each unit at wc_levels_for(dims, L)):
    budget_L          wc_forward_levels_budget, every unit's max_pairs = the pairs
                      leveltol_L keeps of it, so the two sizes match
    leveltol_L        wc_forward_levels_tol, every unit's tolerance = --frac times its RMS
    levels_thresh_L   wc_forward_levels with an explicit threshold: the same dense
                      staging, level passes and emit, no selection (a)
Medians of --steps calls each after --warmup, then one profiled pass per leg for
the stage times (WC_STAGE_TOL: the select or the bins + pick, and the mask pass);
per leg also the kept pairs, the payload bytes and the actual RMSE of its round
trip (wc_inverse_levels + wc_rmse: root mean square over units), which compares
the two selection rules at equal size.

Estimate from bytes, written before the first run (N = the batch's cells, fp32
coefficients; rates of profiles/r06/experiments/gpu_bw_mix.txt, plain accesses):
over (a) the select reads the final array three times, 4 B per coefficient each
at the read-only 5.87 TB/s, and the mask pass reads it again and writes back the
16-B groups it changed, 4 to 8 B per coefficient.  C2 (N = 268.4 M): 3 x 1.074 GB
= 0.549 ms for the select (0.183 ms per digit; the first digit should cost what
the leveltol bin pass does, 0.47 ms at L = 3, since its LDS atomics and not the
read bound it) plus 0.183 to 0.424 ms for the mask pass.  A unit of at most
WC_OPT_TOL_SOLO_TILES flat tiles (C2: every unit, 1 MiB each) takes its three
digits in one workgroup and one launch: its second and third read may hit in
the caches.

    python tools/bench_budget.py --steps 30 --warmup 5 --out profiles/r13/budget.json
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
    read = 4.0 * ncells / 1e9 / READ_TB_S
    return {"select_digit": round(read, 4), "select_three_digits": round(3 * read, 4),
            "mask_all_stored": round(8.0 * ncells / 1e9 / MIX_TB_S, 4), "mask_nothing_stored": round(read, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frac", type=float, default=0.01, help="each unit's tolerance as a fraction of its RMS")
    ap.add_argument("--thresh", type=float, default=0.35, help="the explicit threshold of the levels_thresh legs")
    ap.add_argument("--levels", default="1,2,3,4", help="the L of the legs (a kernel trace of one L)")
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
        raise SystemExit("bench_budget.py needs a HIP device")
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
    lv = {L: [capi.levels_for(units[i].nx, units[i].ny, units[i].nz, L) for i in range(n)] for L in (1, 2, 3, 4)}
    cap = capi.payload_bound(units, n)
    pay = torch.empty(cap, dtype=torch.uint8, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    kept = torch.zeros(n, dtype=torch.int32, device=dev)
    thresh = torch.zeros(n * capi.WC_MAX_LEVELS, dtype=torch.float32, device=dev)
    bound = torch.zeros(n, dtype=torch.float64, device=dev)
    key = torch.zeros(n, dtype=torch.int32, device=dev)
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

    # every unit's budget: what the tolerance mode keeps of it at this L
    pairs = {}
    for L in Ls:
        leveltol(L)()
        ctx.synchronize()
        pairs[L] = kept.cpu().numpy().view(np.uint32).copy()

    def budget(L):
        return lambda: ctx.forward_levels_budget(cells.data_ptr(), dtype, units, n, lv[L], pairs[L], *outs,
                                                 thresh.data_ptr(), key.data_ptr())

    fwd = {}
    for L in Ls:
        fwd[f"budget_L{L}"] = budget(L)
        fwd[f"leveltol_L{L}"] = leveltol(L)
        fwd[f"levels_thresh_L{L}"] = levels_thresh(L)

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
        L = int(name[-1])
        ctx.profile_enable(True)
        fn()
        ctx.synchronize()
        st = {k: round(v[0], 4) for k, v in ctx.profile_read().items()}
        ctx.profile_enable(False)
        stages[name] = st
        ctx.inverse_levels(pay.data_ptr(), off.data_ptr(), units, n, lv[L], regen.data_ptr())
        ctx.rmse(cells.data_ptr(), dtype, regen.data_ptr(), units, n, rmse.data_ptr())
        ctx.synchronize()
        k = kept.cpu().numpy().view(np.uint32)
        legs[name] = {"kept_pairs": int(k.sum()), "payload_bytes": 20 * n + 8 * int(k.sum()),
                      "rmse": math.sqrt(float((rmse * rmse).mean().item())),
                      "tol_share_of_stages": round(st.get("tol", 0.0) / max(sum(st.values()), 1e-9), 4)}
        if name.startswith("budget"):
            legs[name]["units_over_budget"] = int((k > pairs[L]).sum())
            legs[name]["pairs_below_budget"] = int((pairs[L].astype(np.int64) - k).sum())  # dropped ties

    med = {k: statistics.median(v) for k, v in times.items()}
    res = {
        "bench": "budget", "workload": args.workload, "units": n, "cells": ncells, "dtype": wl["dtype"],
        "steps": args.steps, "warmup": args.warmup, "frac": args.frac, "thresh": args.thresh,
        "ms_median": {k: round(v, 4) for k, v in med.items()},
        "ms_min": {k: round(min(v), 4) for k, v in times.items()},
        "ms_p10": {k: round(sorted(v)[int(0.1 * (len(v) - 1))], 4) for k, v in times.items()},
        "ms_p90": {k: round(sorted(v)[int(0.9 * (len(v) - 1))], 4) for k, v in times.items()},
        "legs": legs, "stage_ms": stages,
        "budget_minus_leveltol_ms": {f"L{L}": round(med[f"budget_L{L}"] - med[f"leveltol_L{L}"], 4) for L in Ls},
        "budget_minus_levels_thresh_ms": {f"L{L}": round(med[f"budget_L{L}"] - med[f"levels_thresh_L{L}"], 4)
                                          for L in Ls},
        "rmse_budget_over_leveltol": {f"L{L}": round(legs[f"budget_L{L}"]["rmse"] /
                                                    max(legs[f"leveltol_L{L}"]["rmse"], 1e-300), 4) for L in Ls},
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
