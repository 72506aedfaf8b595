#!/usr/bin/env python3
"""Cost of thinning payloads in the compressed domain, one library build.

On a bench_workloads shape (default C2: 1024 x 64^3 fp64), device buffers, the
context's own stream, host clock around call + wc_synchronize, alternating, for
each L of --levels (each unit at wc_levels_for(dims, L)).  The input F_L is the
batch's payload at thresh = 0 (wc_forward_levels); every unit's budget K is the
pairs wc_forward_levels_tol keeps of it at --frac times its RMS:
    thin_budget_L     wc_thin_budget(F_L, K)
    thin_thresh_L     wc_thin_thresh(F_L, the per-level thresholds thin_budget found)
    route_today_L     wc_inverse_levels(F_L) + wc_forward_levels_budget(cells, K): the
                      only way to the same size before this call existed
    thin_again_L      wc_thin_budget(the thinned payload, K / 2): an input of the
                      size the tolerance mode reaches, the case the call is for
    route_again_L     the route of today on that input: wc_inverse_levels(the thinned
                      payload) + wc_forward_levels_budget(cells, K / 2)
Medians of --steps calls each after --warmup.  Per L also: the input's and the
results' pairs; whether thin_budget's bytes equal wc_forward_levels_budget's on
the original cells, unit by unit (the identity: the input holds every
candidate); the RMSE of both against the original cells.

Byte model, written before the first run (P = the input's pairs, Q = the kept
ones): the scan reads 8 P and writes 8 P ({key, pos}); the select reads 8 P three
times (a solo unit's second and third read may hit in the caches); the compaction
reads 8 P of scratch and the values' 8 P, and writes 8 Q; the difference pass
reads and writes 4 Q each: 56 P + 16 Q bytes, reported against 8 TB/s.  The
threshold form has no select: 32 P + 16 Q.

    python tools/bench_thin.py --steps 20 --warmup 3 --out profiles/r18/thin.json
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

PEAK_TB_S = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frac", type=float, default=0.01, help="each unit's tolerance as a fraction of its RMS")
    ap.add_argument("--levels", default="1,3")
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
        raise SystemExit("bench_thin.py needs a HIP device")
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
    cap = capi.payload_bound(units, n)

    def buffers(nbytes):
        return (torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev),
                torch.zeros(n, dtype=torch.int32, device=dev))

    full, slots, direct = buffers(cap), buffers(cap), buffers(cap)
    thresh = torch.zeros(n * capi.WC_MAX_LEVELS, dtype=torch.float32, device=dev)
    key = torch.zeros(n, dtype=torch.int32, device=dev)
    bound = torch.zeros(n, dtype=torch.float64, device=dev)
    regen = torch.empty(max(extent, 1), dtype=torch.float32, device=dev)
    rmse = torch.zeros(n, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx = capi.Context(0)

    def ptrs(b, nbytes):
        return b[0].data_ptr(), nbytes, b[1].data_ptr(), b[2].data_ptr()

    def kept_of(b):
        return b[2].cpu().numpy().view(np.uint32).copy()

    def unit_rmse(b, lv):
        ctx.inverse_levels(b[0].data_ptr(), b[1].data_ptr(), units, n, lv, regen.data_ptr())
        ctx.rmse(cells.data_ptr(), dtype, regen.data_ptr(), units, n, rmse.data_ptr())
        ctx.synchronize()
        return math.sqrt(float((rmse * rmse).mean().item()))

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    res_ms, res_min, res_p10, res_p90, legs = {}, {}, {}, {}, {}
    for L in Ls:
        lv = [capi.levels_for(units[i].nx, units[i].ny, units[i].nz, L) for i in range(n)]
        ctx.forward_levels_tol(cells.data_ptr(), dtype, units, n, lv, tol, *ptrs(slots, cap), thresh.data_ptr(),
                               bound.data_ptr())
        ctx.synchronize()
        K = kept_of(slots)
        ctx.forward_levels(cells.data_ptr(), dtype, units, n, lv, 0.0, 0.0, *ptrs(full, cap))
        ctx.synchronize()
        P = int(kept_of(full).astype(np.int64).sum())
        tcap = capi.thin_bound(units, n, K)
        thin, half = buffers(tcap), buffers(capi.thin_bound(units, n, K // 2))
        hcap = capi.thin_bound(units, n, K // 2)
        torch.cuda.synchronize()

        def thin_budget():
            ctx.thin_budget(full[0].data_ptr(), full[1].data_ptr(), units, n, lv, K, *ptrs(thin, tcap), thresh.data_ptr(),
                            key.data_ptr())

        thin_budget()
        ctx.synchronize()
        th = thresh.cpu().numpy().reshape(n, capi.WC_MAX_LEVELS).copy()
        Q = int(kept_of(thin).astype(np.int64).sum())

        def thin_thresh():
            ctx.thin_thresh(full[0].data_ptr(), full[1].data_ptr(), units, n, lv, th, *ptrs(slots, cap))

        def route_today():
            ctx.inverse_levels(full[0].data_ptr(), full[1].data_ptr(), units, n, lv, regen.data_ptr())
            ctx.forward_levels_budget(regen.data_ptr(), capi.WC_F32, units, n, lv, K, *ptrs(direct, cap))

        def thin_again():
            ctx.thin_budget(thin[0].data_ptr(), thin[1].data_ptr(), units, n, lv, K // 2, *ptrs(half, hcap))

        def route_again():
            ctx.inverse_levels(thin[0].data_ptr(), thin[1].data_ptr(), units, n, lv, regen.data_ptr())
            ctx.forward_levels_budget(regen.data_ptr(), capi.WC_F32, units, n, lv, K // 2, *ptrs(direct, cap))

        fns = {f"thin_budget_L{L}": thin_budget, f"thin_thresh_L{L}": thin_thresh, f"route_today_L{L}": route_today,
               f"thin_again_L{L}": thin_again, f"route_again_L{L}": route_again}
        times = {k: [] for k in fns}
        for step in range(args.warmup + args.steps):
            for name, fn in fns.items():  # alternating: drift hits every variant alike
                dt = timed(fn)
                if step >= args.warmup:
                    times[name].append(dt)
        for k, v in times.items():
            res_ms[k] = round(statistics.median(v), 4)
            res_min[k] = round(min(v), 4)
            res_p10[k] = round(sorted(v)[int(0.1 * (len(v) - 1))], 4)
            res_p90[k] = round(sorted(v)[int(0.9 * (len(v) - 1))], 4)

        # the identity: the budgeted forward of the original cells, unit by unit
        thin_budget()
        ctx.forward_levels_budget(cells.data_ptr(), dtype, units, n, lv, K, *ptrs(direct, cap))
        ctx.synchronize()
        tp, to, tk = thin[0].cpu().numpy(), thin[1].cpu().numpy().view(np.uint64), kept_of(thin)
        dp, do, dk = direct[0].cpu().numpy(), direct[1].cpu().numpy().view(np.uint64), kept_of(direct)
        same = sum(capi.unit_payload(tp, to, tk, i) == capi.unit_payload(dp, do, dk, i) for i in range(n))
        r_thin, r_direct = unit_rmse(thin, lv), unit_rmse(direct, lv)
        thin_thresh()
        ctx.synchronize()
        Qt = int(kept_of(slots).astype(np.int64).sum())
        thin_again()
        ctx.synchronize()
        Qh = int(kept_of(half).astype(np.int64).sum())
        model_b, model_t, model_h = 56 * P + 16 * Q, 32 * P + 16 * Qt, 56 * Q + 16 * Qh
        legs[f"L{L}"] = {
            "input_pairs": P, "budget_pairs": int(K.astype(np.int64).sum()), "thin_budget_pairs": Q,
            "thin_thresh_pairs": Qt, "thin_again_pairs": Qh, "units_identical_to_direct_budget": int(same),
            "rmse_thin": r_thin, "rmse_direct": r_direct, "rmse_bits_equal": r_thin == r_direct,
            "model_bytes": {"thin_budget": model_b, "thin_thresh": model_t, "thin_again": model_h},
            "model_fraction_of_peak": {
                "thin_budget": round(model_b / (res_ms[f"thin_budget_L{L}"] * 1e-3) / (PEAK_TB_S * 1e12), 4),
                "thin_thresh": round(model_t / (res_ms[f"thin_thresh_L{L}"] * 1e-3) / (PEAK_TB_S * 1e12), 4),
                "thin_again": round(model_h / (res_ms[f"thin_again_L{L}"] * 1e-3) / (PEAK_TB_S * 1e12), 4)},
            "scratch_bytes": 12 * 4096 * sum(-(-s // 4096) for s in sizes),
        }
        del thin, half

    res = {"bench": "thin", "workload": args.workload, "units": n, "cells": ncells, "dtype": wl["dtype"],
           "steps": args.steps, "warmup": args.warmup, "frac": args.frac, "ms_median": res_ms, "ms_min": res_min,
           "ms_p10": res_p10, "ms_p90": res_p90, "legs": legs, "peak_tb_s_assumed": PEAK_TB_S,
           "device": torch.cuda.get_device_name(0), "library": capi.load_library().wc_version().decode()}
    line = json.dumps(res)
    print(line)
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
