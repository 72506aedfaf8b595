#!/usr/bin/env python3
"""Cost of the RMSE-tolerance mode against the reference rule, one library build.

On a bench_workloads shape (default C2: 1024 x 64^3 fp64), device buffers, the
context's own stream, host clock around call + wc_synchronize, alternating:
  (a) wc_forward_stage(NULL) + wc_forward_emit   dense staging, reference keep rule
  (b) wc_forward_tol                             dense staging, per-unit bins + pick, emit
  (d) wc_forward                                 the default path (sparse staging), for scale
Medians of --steps calls each after --warmup, then one profiled pass for the
per-stage times (WC_STAGE_TOL among them).  Expectation from bytes: (b) - (a) is
one more read of the coefficient scratch, 4 B per cell.  Prints one JSON line;
--out FILE also writes it there.

    python tools/bench_tol.py --steps 30 --warmup 5 --out profiles/r07/tol.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tol", type=float, default=0.05, help="RMSE tolerance of every unit")
    ap.add_argument("--read-tb-s", type=float, default=5.87,
                    help="plain streaming read bandwidth (profiles/r06/experiments/gpu_bw_mix.txt)")
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
        raise SystemExit("bench_tol.py needs a HIP device")
    dev = torch.device("cuda", 0)
    wl = bw.WORKLOADS[args.workload]
    units_py = wl["units"]()
    cells, offsets, extent = bw.synth_cells(torch, dev, units_py, wl["dtype"])
    units, n, _ = bw.units_array(capi, units_py, offsets)
    dtype = capi.WC_F64 if wl["dtype"] == "f64" else capi.WC_F32
    keep = float(np.float32(wl["keep"]))
    tol = np.full(n, args.tol, np.float64)
    cap = capi.payload_bound(units, n)
    pay = torch.empty(cap, dtype=torch.uint8, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    kept = torch.zeros(n, dtype=torch.int32, device=dev)
    bound = torch.zeros(n, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx = capi.Context(0)
    outs = (pay.data_ptr(), cap, off.data_ptr(), kept.data_ptr())

    def run_a():
        ctx.forward_stage(cells.data_ptr(), dtype, units, n, None)
        ctx.forward_emit(units, n, keep, None, *outs)

    def run_b():
        ctx.forward_tol(cells.data_ptr(), dtype, units, n, tol, *outs, None, bound.data_ptr())

    def run_d():
        ctx.forward(cells.data_ptr(), dtype, units, n, keep, *outs)

    variants = {"stage_emit_keep": run_a, "forward_tol": run_b, "forward_default": run_d}
    times = {k: [] for k in variants}
    kept_frac = {}
    for step in range(args.warmup + args.steps):
        for name, fn in variants.items():  # alternating: drift hits every variant alike
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if step >= args.warmup:
                times[name].append(dt)
            elif step == 0:
                kept_frac[name] = float(kept.sum().item()) / float(sum(u.cells for u in units_py))
    stages = {}
    ctx.profile_enable(True)
    for name, fn in variants.items():
        fn()
        ctx.synchronize()
        stages[name] = {k: round(v[0], 4) for k, v in ctx.profile_read().items()}
    ctx.profile_enable(False)
    ncells = sum(u.cells for u in units_py)
    med = {k: statistics.median(v) for k, v in times.items()}
    extra_gb = 4.0 * ncells / 1e9
    est_ms = extra_gb / args.read_tb_s  # GB / (TB/s) = ms
    res = {
        "bench": "tol", "workload": args.workload, "units": n, "cells": ncells, "dtype": wl["dtype"],
        "steps": args.steps, "warmup": args.warmup, "tol": args.tol, "keep": keep,
        "ms_median": {k: round(v, 4) for k, v in med.items()},
        "ms_min": {k: round(min(v), 4) for k, v in times.items()},
        "ms_p90": {k: round(sorted(v)[int(0.9 * (len(v) - 1))], 4) for k, v in times.items()},
        "kept_fraction": {k: round(v, 5) for k, v in kept_frac.items()},
        "stage_ms": stages,
        "tol_minus_keep_ms": round(med["forward_tol"] - med["stage_emit_keep"], 4),
        "extra_read_gb": round(extra_gb, 4), "read_tb_s_assumed": args.read_tb_s,
        "estimate_ms": round(est_ms, 4),
        "bound_max": float(bound.max().item()),
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
