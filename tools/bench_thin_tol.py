#!/usr/bin/env python3
"""Cost of thinning and splitting payloads to an RMSE tolerance in the compressed
domain, one library build.

On a bench_workloads shape (default C2: 1024 x 64^3 fp64), device buffers, the
context's own stream, host clock around call + wc_synchronize, alternating, for
each L of --levels (each unit at wc_levels_for(dims, L)).  Two inputs per L: T_L,
the payloads wc_forward_levels_tol writes at --frac0 times each unit's RMS (what an
archive holds), and F_L, the payloads at thresh = 0 (every candidate).  Both are
thinned at --frac1 times the RMS:
    thin_tol_<in>_L       wc_thin_tol(input, tol1)
    split_tol_<in>_L      wc_split_tol(input, tol1)
    thin_thresh_<in>_L    wc_thin_thresh(input, the thresholds thin_tol found): the
                          floor, thin_tol is this plus the bin pass and the walk
    thin_budget_<in>_L    wc_thin_budget(input, the kept counts thin_tol reached): one
                          bin pass against three digit passes
    route_<in>_L          wc_inverse_levels(input) + wc_forward_levels_tol(cells, tol1):
                          the only way to a tolerance before this call existed
Medians of --steps calls each after --warmup.  Per L and input also: the pairs in
and out, the sum of the bounds, the actual RMSE of the thinned payloads against the
original cells beside sqrt(tol0^2 + bound1^2), and how many units of thin_tol are
byte for byte the route's.  On F_L the rule's identity is asserted: wc_thin_tol's
bytes, thresholds and bounds equal wc_forward_levels_tol's on the original cells.

Byte model, written before the first run (P = the input's pairs, Q = the kept
ones): the scan reads 8 P and writes 8 P ({key, pos}); the bin pass reads 8 P once;
the compaction reads 8 P of scratch and the values' 8 P, and writes 8 Q; the
difference pass reads and writes 4 Q each: 40 P + 16 Q bytes, against 56 P + 16 Q
of the budget form and 32 P + 16 Q of the threshold form, reported against 8 TB/s.

    python tools/bench_thin_tol.py --steps 20 --warmup 3 --out profiles/r20/thin_tol.json
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
    ap.add_argument("--frac0", type=float, default=0.01, help="the archive's tolerance as a fraction of each unit's RMS")
    ap.add_argument("--frac1", type=float, default=0.03, help="the thinning's tolerance as a fraction of each unit's RMS")
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
        raise SystemExit("bench_thin_tol.py needs a HIP device")
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
    tol0, tol1 = args.frac0 * rms, args.frac1 * rms
    cap = capi.payload_bound(units, n)
    assert cap == capi.thin_bound(units, n, None)

    def buffers(nbytes):
        return (torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev),
                torch.zeros(n, dtype=torch.int32, device=dev))

    inputs = {"T": buffers(cap), "F": buffers(cap)}
    thin, base, rest, slots, direct = buffers(cap), buffers(cap), buffers(cap), buffers(cap), buffers(cap)

    def selection():
        return (torch.zeros(n * capi.WC_MAX_LEVELS, dtype=torch.float32, device=dev),
                torch.zeros(n, dtype=torch.float64, device=dev))

    sel_thin, sel_split, sel_direct = selection(), selection(), selection()
    regen = torch.empty(max(extent, 1), dtype=torch.float32, device=dev)
    rmse = torch.zeros(n, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx = capi.Context(0)

    def ptrs(b):
        return b[0].data_ptr(), cap, b[1].data_ptr(), b[2].data_ptr()

    def kept_of(b):
        return b[2].cpu().numpy().view(np.uint32).copy()

    def payloads(b):
        p, o, k = b[0].cpu().numpy(), b[1].cpu().numpy().view(np.uint64), kept_of(b)
        return [capi.unit_payload(p, o, k, i) for i in range(n)]

    def unit_rmse(b, lv):
        ctx.inverse_levels(b[0].data_ptr(), b[1].data_ptr(), units, n, lv, regen.data_ptr())
        ctx.rmse(cells.data_ptr(), dtype, regen.data_ptr(), units, n, rmse.data_ptr())
        ctx.synchronize()
        return rmse.cpu().numpy().copy()

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    res_ms, res_min, res_p10, res_p90, legs = {}, {}, {}, {}, {}
    for L in Ls:
        lv = [capi.levels_for(units[i].nx, units[i].ny, units[i].nz, L) for i in range(n)]
        ctx.forward_levels_tol(cells.data_ptr(), dtype, units, n, lv, tol0, *ptrs(inputs["T"]))
        ctx.forward_levels(cells.data_ptr(), dtype, units, n, lv, 0.0, 0.0, *ptrs(inputs["F"]))
        ctx.synchronize()
        for tag, src in inputs.items():
            P = int(kept_of(src).astype(np.int64).sum())

            def thin_tol():
                ctx.thin_tol(src[0].data_ptr(), src[1].data_ptr(), units, n, lv, tol1, *ptrs(thin), sel_thin[0].data_ptr(),
                             sel_thin[1].data_ptr())

            thin_tol()
            ctx.synchronize()
            th = sel_thin[0].cpu().numpy().reshape(n, capi.WC_MAX_LEVELS).copy()
            bound1 = sel_thin[1].cpu().numpy().copy()
            K = kept_of(thin)
            Q = int(K.astype(np.int64).sum())
            bcap = capi.thin_bound(units, n, K)
            budget = (torch.empty(bcap, dtype=torch.uint8, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev),
                      torch.zeros(n, dtype=torch.int32, device=dev))
            torch.cuda.synchronize()

            def split_tol():
                ctx.split_tol(src[0].data_ptr(), src[1].data_ptr(), units, n, lv, tol1, *ptrs(base), *ptrs(rest),
                              sel_split[0].data_ptr(), sel_split[1].data_ptr())

            def thin_thresh():
                ctx.thin_thresh(src[0].data_ptr(), src[1].data_ptr(), units, n, lv, th, *ptrs(slots))

            def thin_budget():
                ctx.thin_budget(src[0].data_ptr(), src[1].data_ptr(), units, n, lv, K, budget[0].data_ptr(), bcap,
                                budget[1].data_ptr(), budget[2].data_ptr())

            def route():
                ctx.inverse_levels(src[0].data_ptr(), src[1].data_ptr(), units, n, lv, regen.data_ptr())
                ctx.forward_levels_tol(regen.data_ptr(), capi.WC_F32, units, n, lv, tol1, *ptrs(direct))

            fns = {f"thin_tol_{tag}_L{L}": thin_tol, f"split_tol_{tag}_L{L}": split_tol,
                   f"thin_thresh_{tag}_L{L}": thin_thresh, f"thin_budget_{tag}_L{L}": thin_budget,
                   f"route_{tag}_L{L}": route}
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

            for fn in fns.values():
                fn()
            ctx.synchronize()
            tp = payloads(thin)
            same_route = sum(a == b for a, b in zip(tp, payloads(direct)))
            same_thresh = sum(a == b for a, b in zip(tp, payloads(slots)))
            same_base = sum(a == b for a, b in zip(tp, payloads(base)))
            Qb = int(kept_of(budget).astype(np.int64).sum())
            R = int(kept_of(rest).astype(np.int64).sum())
            assert same_thresh == n and same_base == n, (same_thresh, same_base)
            if tag == "F":  # the rule's identity: the input holds every candidate and the cells are NaN-free
                ctx.forward_levels_tol(cells.data_ptr(), dtype, units, n, lv, tol1, *ptrs(direct), sel_direct[0].data_ptr(),
                                       sel_direct[1].data_ptr())
                ctx.synchronize()
                assert tp == payloads(direct), "wc_thin_tol(thresh = 0 payload) differs from wc_forward_levels_tol"
                assert sel_thin[0].cpu().numpy().tobytes() == sel_direct[0].cpu().numpy().tobytes()
                assert sel_thin[1].cpu().numpy().tobytes() == sel_direct[1].cpu().numpy().tobytes()
            actual = unit_rmse(thin, lv)
            t0 = tol0 if tag == "T" else np.zeros(n)
            composed = np.sqrt(t0 * t0 + bound1 * bound1)
            mb, mt, mk = 40 * P + 16 * Q, 32 * P + 16 * Q, 56 * P + 16 * Qb
            legs[f"{tag}_L{L}"] = {
                "input_pairs": P, "thin_tol_pairs": Q, "rest_pairs": R, "thin_budget_pairs": Qb,
                "units_identical_to_route": int(same_route), "units_identical_to_thin_thresh": int(same_thresh),
                "base_identical_to_thin_tol": int(same_base),
                "identical_to_forward_levels_tol_on_the_cells": True if tag == "F" else None,
                "bound_over_tol1_mean": float(np.mean(bound1 / np.maximum(tol1, 1e-300))),
                "rmse_actual_rms": float(math.sqrt(float((actual * actual).mean()))),
                "rmse_composed_rms": float(math.sqrt(float((composed * composed).mean()))),
                "units_within_composed_bound": int((actual <= composed * (1 + 1e-3)).sum()),
                "model_bytes": {"thin_tol": mb, "thin_thresh": mt, "thin_budget": mk},
                "model_fraction_of_peak": {
                    "thin_tol": round(mb / (res_ms[f"thin_tol_{tag}_L{L}"] * 1e-3) / (PEAK_TB_S * 1e12), 4),
                    "thin_thresh": round(mt / (res_ms[f"thin_thresh_{tag}_L{L}"] * 1e-3) / (PEAK_TB_S * 1e12), 4),
                    "thin_budget": round(mk / (res_ms[f"thin_budget_{tag}_L{L}"] * 1e-3) / (PEAK_TB_S * 1e12), 4)},
                "scratch_bytes": {"thin": 12 * 4096 * sum(-(-s // 4096) for s in sizes),
                                  "split": 16 * 4096 * sum(-(-s // 4096) for s in sizes)},
            }
            del budget

    res = {"bench": "thin_tol", "workload": args.workload, "units": n, "cells": ncells, "dtype": wl["dtype"],
           "steps": args.steps, "warmup": args.warmup, "frac0": args.frac0, "frac1": args.frac1, "ms_median": res_ms,
           "ms_min": res_min, "ms_p10": res_p10, "ms_p90": res_p90, "legs": legs, "peak_tb_s_assumed": PEAK_TB_S,
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
