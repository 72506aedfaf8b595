#!/usr/bin/env python3
"""Cost of the reduced-resolution decode against the full inverse of the same payloads.

On a bench_workloads shape (default C2: 1024 x 64^3 fp64), device buffers, the
context's own stream, host clock around call + wc_synchronize, alternating:
  payloads at L = 3 (wc_forward_levels, the workload's keep)
    coarse_L3_r{1,2,3}   wc_inverse_coarse at r = 1, 2, 3
    inverse_levels3      wc_inverse_levels of the same payloads
  payloads at L = 1 (wc_forward, the reference's format)
    coarse_L1_r1         wc_inverse_coarse at r = 1 (the corner is the result)
    inverse_default      wc_inverse of the same payloads (row-indexed)
Medians of --steps calls each after --warmup, then one profiled pass per leg for
the stage times (decode: the clears and the corner decode; levels: the passes;
inverse: the final one-level inverse).

Estimate from bytes, written before the first run (n units of W^3 = N cells
each, P kept pairs in all, (w, h, d) = W >> r, c = n w^3 corner coefficients;
rates of profiles/r06/experiments/gpu_bw_mix.txt, plain accesses: read only
5.87 TB/s, write only 5.19, the 1:1 mix 5.06):
  payload     the pairs up to the corner's end, end = ((w-1) W + (w-1)) W + w,
              taking the pairs as spread evenly over the flat positions:
              8 P end / N bytes, read
  scratch     the compact corners cleared (4 c, written), scattered into (4 c at
              most, written) and read back by what follows (counted there)
  passes      levels L-r..2 of the derived units, 16 B per coefficient of each
              sub-box: 16 c / 8^(l-1), the 1:1 mix
  inverse     the final one-level inverse reads 4 c and writes the 4 c coarse
              cells (r < L); with r = L the scatter itself writes the cells
  C2 (n = 1024, W = 64, P = 56.75 M at L = 3, 81.35 M at L = 1, profiles/r08/levels.json):
    L3 r1  end/N 0.492: 223 + 134 + 134 + 67 + 268 MB = 0.83 GB   0.156 ms
    L3 r2  end/N 0.238: 108 + 17 + 17 + 0 + 34 MB    = 0.18 GB   0.032 ms
    L3 r3  end/N 0.111:  50 + 2 + 2 MB               = 0.06 GB   0.009 ms
    L1 r1  end/N 0.492: 320 + 134 + 134 MB           = 0.59 GB   0.106 ms
  against wc_inverse_levels at L = 3: payload 454 MB, the dense array written
  (1.07 GB), the passes (0.60 GB), the inverse (2.15 GB) = 4.3 GB, 0.98 ms
  measured.  The r = 2 and r = 3 legs are 6 to 8 stream operations (two clears,
  the corner decode, the passes, the inverse) of a few microseconds each: their
  byte estimates are below what the launches alone cost, so expect those legs
  to be bound by launch latency, not by bytes.
(After the first run the units with r = L were moved off the direct scatter: they
decode into the compact corner and k_corner_box copies it to Box3D order, 8 c
more bytes that this estimate, left as written, does not hold.)

    python tools/bench_coarse.py --steps 30 --warmup 5 --out profiles/r09/coarse.json
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

READ_TB_S = 5.87   # read only, plain
WRITE_TB_S = 5.19  # write only, plain
MIX_TB_S = 5.06    # 1:1 reads and writes, plain


def estimate(units, pairs: int, L: int, r: int):
    """-> (GB moved, ms) of wc_inverse_coarse by the model in the header."""
    ncells = sum(u.nx * u.ny * u.nz for u in units)
    pay = clear = passes = inv = 0.0
    for u in units:
        N = u.nx * u.ny * u.nz
        w, h, d = u.nx >> r, u.ny >> r, u.nz >> r
        if not N:
            continue
        end = ((w - 1) * u.ny + (h - 1)) * u.nz + d
        pay += 8.0 * pairs * (N / ncells) * end / N
        c = w * h * d
        clear += 4.0 * c
        passes += sum(16.0 * c / 8 ** (l - 1) for l in range(2, L - r + 1))
        inv += 8.0 * c if r < L else 0.0
    gb = (pay + 2 * clear + passes + inv) / 1e9
    ms = (pay / READ_TB_S + 2 * clear / WRITE_TB_S + (passes + inv) / MIX_TB_S) / 1e9
    return gb, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
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
        raise SystemExit("bench_coarse.py needs a HIP device")
    dev = torch.device("cuda", 0)
    wl = bw.WORKLOADS[args.workload]
    units_py = wl["units"]()
    cells, offsets, extent = bw.synth_cells(torch, dev, units_py, wl["dtype"])
    units, n, _ = bw.units_array(capi, units_py, offsets)
    dtype = capi.WC_F64 if wl["dtype"] == "f64" else capi.WC_F32
    keep = float(np.float32(wl["keep"]))
    ncells = sum(u.cells for u in units_py)
    L3 = [capi.levels_for(units[i].nx, units[i].ny, units[i].nz, 3) for i in range(n)]
    if set(L3) != {3}:
        raise SystemExit("bench_coarse.py needs units that admit three levels")
    cap = capi.payload_bound(units, n)
    pay = {k: torch.empty(cap, dtype=torch.uint8, device=dev) for k in ("L3", "L1")}
    off = {k: torch.zeros(n + 1, dtype=torch.int64, device=dev) for k in ("L3", "L1")}
    kept = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in ("L3", "L1")}
    regen = torch.empty(max(extent, 1), dtype=torch.float32, device=dev)
    coarse = {r: capi.coarse_units(units, n, r) for r in (1, 2, 3)}
    cout = torch.empty(max(coarse[1][1], 1), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx = capi.Context(0)
    ctx.forward_levels(cells.data_ptr(), dtype, units, n, L3, keep, None, pay["L3"].data_ptr(), cap,
                       off["L3"].data_ptr(), kept["L3"].data_ptr())
    ctx.forward(cells.data_ptr(), dtype, units, n, keep, pay["L1"].data_ptr(), cap, off["L1"].data_ptr(),
                kept["L1"].data_ptr())
    ctx.synchronize()
    pairs = {k: int(kept[k].sum().item()) for k in kept}

    def coarse_leg(which, levels, r):
        return lambda: ctx.inverse_coarse(pay[which].data_ptr(), off[which].data_ptr(), units, n, levels, r,
                                          coarse[r][0], cout.data_ptr())

    groups = {
        "L3": {"coarse_L3_r1": coarse_leg("L3", L3, 1), "coarse_L3_r2": coarse_leg("L3", L3, 2),
               "coarse_L3_r3": coarse_leg("L3", L3, 3),
               "inverse_levels3": lambda: ctx.inverse_levels(pay["L3"].data_ptr(), off["L3"].data_ptr(), units, n, L3,
                                                             regen.data_ptr())},
        "L1": {"coarse_L1_r1": coarse_leg("L1", None, 1),
               "inverse_default": lambda: ctx.inverse(pay["L1"].data_ptr(), off["L1"].data_ptr(), units, n,
                                                      regen.data_ptr())},
    }

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

    times, stages = {}, {}
    for legs in groups.values():
        for step in range(args.warmup + args.steps):
            for name, fn in legs.items():  # alternating: drift hits every leg alike
                dt = timed(fn)
                if step >= args.warmup:
                    times.setdefault(name, []).append(dt)
        for name, fn in legs.items():
            stages[name] = profiled(fn)

    med = {k: statistics.median(v) for k, v in times.items()}
    full = {"coarse_L3_r1": "inverse_levels3", "coarse_L3_r2": "inverse_levels3", "coarse_L3_r3": "inverse_levels3",
            "coarse_L1_r1": "inverse_default"}
    est = {"coarse_L3_r1": estimate(units[:n], pairs["L3"], 3, 1), "coarse_L3_r2": estimate(units[:n], pairs["L3"], 3, 2),
           "coarse_L3_r3": estimate(units[:n], pairs["L3"], 3, 3), "coarse_L1_r1": estimate(units[:n], pairs["L1"], 1, 1)}
    res = {
        "bench": "coarse", "workload": args.workload, "units": n, "cells": ncells, "dtype": wl["dtype"],
        "steps": args.steps, "warmup": args.warmup, "keep": keep, "kept_pairs": pairs,
        "ms_median": {k: round(v, 4) for k, v in med.items()},
        "ms_min": {k: round(min(v), 4) for k, v in times.items()},
        "ms_p90": {k: round(sorted(v)[int(0.9 * (len(v) - 1))], 4) for k, v in times.items()},
        "stage_ms": stages,
        "estimate_gb": {k: round(v[0], 4) for k, v in est.items()},
        "estimate_ms": {k: round(v[1], 4) for k, v in est.items()},
        "measured_over_estimate": {k: round(med[k] / est[k][1], 2) for k in est},
        "ratio_to_full_inverse": {k: round(med[k] / med[f], 4) for k, f in full.items()},
        "read_tb_s_assumed": READ_TB_S, "write_tb_s_assumed": WRITE_TB_S, "mix_tb_s_assumed": MIX_TB_S,
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
