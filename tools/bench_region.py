#!/usr/bin/env python3
"""Cost of the sub-box decode against the full inverse of the same payloads.

On a bench_workloads shape (default C2: 1024 x 64^3 fp64), device buffers, the
context's own stream, host clock around call + wc_synchronize, alternating:
  payloads at L = 3 (wc_forward_levels, the workload's keep)
    region_L3_{x,y,z}_r0   wc_inverse_region, an 8-thick slab normal to x, y, z
                           (cells 24..31 of that axis) in every unit, r = 0
    region_L3_{x,y,z}_r1   the same slabs at r = 1
    region_L3_block        one 8^3 block at (24, 24, 24) in every unit, r = 0
    inverse_levels3        wc_inverse_levels of the same payloads
  payloads at L = 1 (wc_forward, the reference's format)
    region_L1_...          the same legs (r = 1: the compact unit is the result)
    inverse_default        wc_inverse of the same payloads (row-indexed)
The full inverse is what a caller who wants the slab has today.  Medians of
--steps calls each after --warmup, then one profiled pass per leg for the stage
times (decode: the clear, the region decode and, at r = L, k_corner_box; levels:
the passes; inverse: the final one-level inverse).

Estimate from bytes, written before the first run (n units of W^3 = N cells each,
P kept pairs in all, c = the regions' cells >> 3r in all; rates of
profiles/r06/experiments/gpu_bw_mix.txt, plain accesses: read only 5.87 TB/s,
write only 5.19, the 1:1 mix 5.06):
  payload     the pairs up to `end` (include/wavelet_amd.h), taking the pairs as
              spread evenly over the flat positions: 8 P end / N bytes, read
  scratch     the compact units cleared (4 c, written) and scattered into (4 c at
              most, written)
  passes      levels L'..2 of the compact units, 16 B per coefficient of each
              sub-box: 16 c / 8^(l-1), the 1:1 mix
  inverse     the final one-level inverse reads 4 c and writes 4 c; at r = L
              k_corner_box moves the same 8 c
  C2 (n = 1024, W = 64, P = 56.75 M at L = 3, 81.35 M at L = 1, profiles/r08/levels.json):
    L3 x r0  end/N 0.750: 340 + 134 + 134 + 75 + 268 MB = 0.95 GB   0.178 ms
    L3 y r0  end/N 0.996: 452 + 611 MB                  = 1.06 GB   0.197 ms
    L3 z r0  end/N 1.000: 454 + 611 MB                  = 1.07 GB   0.197 ms
    L3 x r1  end/N 0.367: 167 + 17 + 17 + 8 + 34 MB     = 0.24 GB   0.043 ms
    L3 y r1  end/N 0.490: 222 + 76 MB                   = 0.30 GB   0.053 ms
    L3 z r1  end/N 0.492: 223 + 76 MB                   = 0.30 GB   0.053 ms
    L3 block end/N 0.746: 339 + 2 + 2 + 1 + 4 MB        = 0.35 GB   0.060 ms
    L1 x r0  end/N 0.750: 488 + 134 + 134 + 268 MB      = 1.02 GB   0.188 ms
    L1 y r0, z r0  end/N 1.0: 650 + 536 MB              = 1.19 GB   0.216 ms
    L1 x r1  end/N 0.242: 157 + 17 + 17 + 34 MB         = 0.22 GB   0.040 ms
    L1 y r1, z r1  end/N 0.49: 318 + 67 MB              = 0.39 GB   0.067 ms
    L1 block end/N 0.746: 486 + 8 MB                    = 0.49 GB   0.085 ms
  against wc_inverse_levels at L = 3, 0.97 ms, and wc_inverse, 0.50 ms
  (profiles/r09/coarse.json).  A slab normal to y or z needs pairs up to the end
  of the array, so its payload term is the whole payload: the slab normal to x
  is the cheap one, as the flat order is x-slowest.  The reduced-resolution
  decode missed such estimates by 2 to 18 times, the more the fewer bytes a leg
  moved: each leg is 5 to 9 stream operations of a few microseconds each, and
  the decode kernel's blocks do their scan whether or not their pairs are kept.

    python tools/bench_region.py --steps 30 --warmup 5 --out profiles/r12/region.json
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


def region_end(dims, L, r, g):
    """`end` of include/wavelet_amd.h for the box dims, L levels, reduction r and region g."""
    n = [v >> r for v in dims]
    o = [v >> r for v in g[:3]]
    s = [v >> r for v in g[3:]]
    if not s[0] * s[1] * s[2]:
        return 0
    last = [(n[a] >> 1) + (o[a] >> 1) + (s[a] >> 1) - 1 if L - r >= 1 else o[a] + s[a] - 1 for a in range(3)]
    return (last[0] * dims[1] + last[1]) * dims[2] + last[2] + 1


def estimate(units, pairs: int, L: int, r: int, g):
    """-> (GB moved, ms) of wc_inverse_region by the model in the header."""
    ncells = sum(u.nx * u.ny * u.nz for u in units)
    pay = clear = passes = inv = 0.0
    for u in units:
        N = u.nx * u.ny * u.nz
        if not N:
            continue
        pay += 8.0 * pairs * (N / ncells) * region_end((u.nx, u.ny, u.nz), L, r, g) / N
        c = (g[3] >> r) * (g[4] >> r) * (g[5] >> r)
        clear += 4.0 * c
        passes += sum(16.0 * c / 8 ** (l - 1) for l in range(2, L - r + 1))
        inv += 8.0 * c
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
        raise SystemExit("bench_region.py needs a HIP device")
    dev = torch.device("cuda", 0)
    wl = bw.WORKLOADS[args.workload]
    units_py = wl["units"]()
    cells, offsets, extent = bw.synth_cells(torch, dev, units_py, wl["dtype"])
    units, n, _ = bw.units_array(capi, units_py, offsets)
    dtype = capi.WC_F64 if wl["dtype"] == "f64" else capi.WC_F32
    keep = float(np.float32(wl["keep"]))
    ncells = sum(u.cells for u in units_py)
    L3 = [capi.levels_for(units[i].nx, units[i].ny, units[i].nz, 3) for i in range(n)]
    if set(L3) != {3} or any(min(units[i].nx, units[i].ny, units[i].nz) < 32 for i in range(n)):
        raise SystemExit("bench_region.py needs units of at least 32 cells an axis that admit three levels")
    cap = capi.payload_bound(units, n)
    pay = {k: torch.empty(cap, dtype=torch.uint8, device=dev) for k in ("L3", "L1")}
    off = {k: torch.zeros(n + 1, dtype=torch.int64, device=dev) for k in ("L3", "L1")}
    kept = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in ("L3", "L1")}
    regen = torch.empty(max(extent, 1), dtype=torch.float32, device=dev)
    W, H, D = units[0].nx, units[0].ny, units[0].nz  # the legs' regions are those of the first unit's box
    if any((units[i].nx, units[i].ny, units[i].nz) != (W, H, D) for i in range(n)):
        raise SystemExit("bench_region.py needs units of one shape")
    shapes = {"x": (24, 0, 0, 8, H, D), "y": (0, 24, 0, W, 8, D), "z": (0, 0, 24, W, H, 8), "block": (24, 24, 24, 8, 8, 8)}
    legs_of = [("x", 0), ("y", 0), ("z", 0), ("x", 1), ("y", 1), ("z", 1), ("block", 0)]
    layout = {}
    for s, r in legs_of:
        regions = capi.make_regions([shapes[s]] * n, n)
        layout[(s, r)] = (regions,) + capi.region_units(units, n, regions, r)
    rout = torch.empty(max(v[2] for v in layout.values()) + 4, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx = capi.Context(0)
    ctx.forward_levels(cells.data_ptr(), dtype, units, n, L3, keep, None, pay["L3"].data_ptr(), cap,
                       off["L3"].data_ptr(), kept["L3"].data_ptr())
    ctx.forward(cells.data_ptr(), dtype, units, n, keep, pay["L1"].data_ptr(), cap, off["L1"].data_ptr(),
                kept["L1"].data_ptr())
    ctx.synchronize()
    pairs = {k: int(kept[k].sum().item()) for k in kept}

    def region_leg(which, levels, s, r):
        regions, out_units, _ = layout[(s, r)]
        return lambda: ctx.inverse_region(pay[which].data_ptr(), off[which].data_ptr(), units, n, levels, r, regions,
                                          out_units, rout.data_ptr())

    def name(which, s, r):
        return f"region_{which}_block" if s == "block" else f"region_{which}_{s}_r{r}"

    groups = {
        "L3": {name("L3", s, r): region_leg("L3", L3, s, r) for s, r in legs_of},
        "L1": {name("L1", s, r): region_leg("L1", None, s, r) for s, r in legs_of},
    }
    groups["L3"]["inverse_levels3"] = lambda: ctx.inverse_levels(pay["L3"].data_ptr(), off["L3"].data_ptr(), units, n,
                                                                 L3, regen.data_ptr())
    groups["L1"]["inverse_default"] = lambda: ctx.inverse(pay["L1"].data_ptr(), off["L1"].data_ptr(), units, n,
                                                          regen.data_ptr())

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
            for leg, fn in legs.items():  # alternating: drift hits every leg alike
                dt = timed(fn)
                if step >= args.warmup:
                    times.setdefault(leg, []).append(dt)
        for leg, fn in legs.items():
            stages[leg] = profiled(fn)

    med = {k: statistics.median(v) for k, v in times.items()}
    full, est, ends = {}, {}, {}
    for which, L, base in (("L3", 3, "inverse_levels3"), ("L1", 1, "inverse_default")):
        for s, r in legs_of:
            full[name(which, s, r)] = base
            est[name(which, s, r)] = estimate(units[:n], pairs[which], L, r, shapes[s])
            ends[name(which, s, r)] = round(region_end((W, H, D), L, r, shapes[s]) / (W * H * D), 4)
    res = {
        "bench": "region", "workload": args.workload, "units": n, "cells": ncells, "dtype": wl["dtype"],
        "steps": args.steps, "warmup": args.warmup, "keep": keep, "kept_pairs": pairs,
        "regions": {k: list(v) for k, v in shapes.items()}, "end_over_cells": ends,
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
