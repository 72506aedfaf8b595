#!/usr/bin/env python3
"""Cost of the progressive layers (wc_split_budget, wc_merge), one library build.

On a bench_workloads shape (default C2: 1024 x 64^3 fp64), device buffers, the
context's own stream, host clock around call + wc_synchronize, alternating, for
each L of --levels (each unit at wc_levels_for(dims, L)).  F_L is the batch's
payload at thresh = 0 (wc_forward_levels); T_L = wc_thin_budget(F_L, K), K per unit
the pairs wc_forward_levels_tol keeps at --frac times its RMS: the tolerance-sized
payload of tools/bench_thin.py.  On either input X (T_L: "tol", F_L: "full"), split
at half its size (K / 2, respectively K):
    split_X_L     wc_split_budget(X, k) -> (base, rest)
    thin_X_L      wc_thin_budget(X, k): the same base without the rest, same run
    merge_X_L     wc_merge(base, rest)
    rewrite_X_L   wc_thin_thresh(canon(X) = merge's result, thresholds 0): a pass that
                  reads and rewrites the same pairs, the yardstick for the merge
Medians of --steps calls each after --warmup.  Per leg also the pair counts and the
identity: the units (of all n) where wc_merge(wc_split_budget(X)) == X byte for
byte and where the split's base equals wc_thin_budget's.

Byte models, written before the first run (P = the input's pairs, Q = the base's,
R = the rest's, Q + R = P here): split = the thinning's 56 P + 16 Q (tools/
bench_thin.py) plus the rest's writes, 8 R in the compaction (value + position)
and 8 R in its difference pass (position read, run written): 56 P + 16 Q + 16 R.
merge = 8 B per input pair read by the scan, 4 B of position written and 4 B read
again, 8 B per output pair written: 24 P.  Not in the merge's model: the value the
place pass reads a second time and the loads of its searches.  Both against 8 TB/s.

    python tools/bench_layers.py --steps 20 --warmup 3 --out profiles/r19/layers.json
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
        raise SystemExit("bench_layers.py needs a HIP device")
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

    full, rest, merged, rewritten = buffers(cap), buffers(cap), buffers(cap), buffers(cap)
    thresh = torch.zeros(n * capi.WC_MAX_LEVELS, dtype=torch.float32, device=dev)
    bound = torch.zeros(n, dtype=torch.float64, device=dev)
    zeros = np.zeros((n, capi.WC_MAX_LEVELS), np.float32)
    torch.cuda.synchronize()
    ctx = capi.Context(0)

    def ptrs(b, nbytes):
        return b[0].data_ptr(), nbytes, b[1].data_ptr(), b[2].data_ptr()

    def kept_of(b):
        return b[2].cpu().numpy().view(np.uint32).copy()

    def same_units(a, b):
        """Units whose serialized bytes in a and in b are equal (compared on the device)."""
        oa, ob = a[1].cpu().numpy().view(np.uint64), b[1].cpu().numpy().view(np.uint64)
        ka, kb = kept_of(a), kept_of(b)
        same = 0
        for i in range(n):
            ln = 20 + 8 * int(ka[i])
            same += int(ka[i] == kb[i] and
                        torch.equal(a[0][int(oa[i]):int(oa[i]) + ln], b[0][int(ob[i]):int(ob[i]) + ln]))
        return same

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    res_ms, res_min, res_p10, res_p90, legs = {}, {}, {}, {}, {}
    for L in Ls:
        lv = [capi.levels_for(units[i].nx, units[i].ny, units[i].nz, L) for i in range(n)]
        ctx.forward_levels_tol(cells.data_ptr(), dtype, units, n, lv, tol, *ptrs(rest, cap), thresh.data_ptr(),
                               bound.data_ptr())
        ctx.synchronize()
        K = kept_of(rest)
        ctx.forward_levels(cells.data_ptr(), dtype, units, n, lv, 0.0, 0.0, *ptrs(full, cap))
        tcap = capi.thin_bound(units, n, K)
        tolp = buffers(tcap)
        ctx.thin_budget(full[0].data_ptr(), full[1].data_ptr(), units, n, lv, K, *ptrs(tolp, tcap))
        ctx.synchronize()
        for tag, X, k in (("tol", tolp, K // 2), ("full", full, K)):
            bcap = capi.split_bound(units, n, k)[0]
            base, thin = buffers(bcap), buffers(bcap)
            torch.cuda.synchronize()
            x = (X[0].data_ptr(), X[1].data_ptr(), units, n, lv)

            def split():
                ctx.split_budget(*x, k, *ptrs(base, bcap), *ptrs(rest, cap))

            def thin_budget():
                ctx.thin_budget(*x, k, *ptrs(thin, bcap))

            def merge():
                ctx.merge(base[0].data_ptr(), base[1].data_ptr(), rest[0].data_ptr(), rest[1].data_ptr(), units, n, lv,
                          *ptrs(merged, cap))

            def rewrite():
                ctx.thin_thresh(merged[0].data_ptr(), merged[1].data_ptr(), units, n, lv, zeros, *ptrs(rewritten, cap))

            fns = {f"split_{tag}_L{L}": split, f"thin_{tag}_L{L}": thin_budget, f"merge_{tag}_L{L}": merge,
                   f"rewrite_{tag}_L{L}": rewrite}
            times = {name: [] for name in fns}
            for step in range(args.warmup + args.steps):
                for name, fn in fns.items():  # alternating: drift hits every variant alike
                    dt = timed(fn)
                    if step >= args.warmup:
                        times[name].append(dt)
            for name, v in times.items():
                res_ms[name] = round(statistics.median(v), 4)
                res_min[name] = round(min(v), 4)
                res_p10[name] = round(sorted(v)[int(0.1 * (len(v) - 1))], 4)
                res_p90[name] = round(sorted(v)[int(0.9 * (len(v) - 1))], 4)
            # the identity and the base, unit by unit
            P = int(kept_of(X).astype(np.int64).sum())
            Q = int(kept_of(base).astype(np.int64).sum())
            R = int(kept_of(rest).astype(np.int64).sum())
            m_split, m_thin, m_merge = 56 * P + 16 * Q + 16 * R, 56 * P + 16 * Q, 24 * P

            def frac(model, name):
                return round(model / (res_ms[name] * 1e-3) / (PEAK_TB_S * 1e12), 4)

            legs[f"{tag}_L{L}"] = {
                "input_pairs": P, "base_pairs": Q, "rest_pairs": R, "merged_pairs": int(kept_of(merged).astype(np.int64).sum()),
                "units_merge_of_split_identical_to_input": same_units(merged, X),
                "units_base_identical_to_thin_budget": same_units(base, thin),
                "units_rewrite_identical_to_input": same_units(rewritten, X),
                "model_bytes": {"split": m_split, "thin_budget": m_thin, "merge": m_merge},
                "model_fraction_of_peak": {"split": frac(m_split, f"split_{tag}_L{L}"),
                                           "thin_budget": frac(m_thin, f"thin_{tag}_L{L}"),
                                           "merge": frac(m_merge, f"merge_{tag}_L{L}")},
                "split_over_thin": round(res_ms[f"split_{tag}_L{L}"] / res_ms[f"thin_{tag}_L{L}"], 3),
                "merge_over_rewrite": round(res_ms[f"merge_{tag}_L{L}"] / res_ms[f"rewrite_{tag}_L{L}"], 3),
            }
            del base, thin
        del tolp

    tiles = sum(-(-s // 4096) for s in sizes)
    res = {"bench": "layers", "workload": args.workload, "units": n, "cells": ncells, "dtype": wl["dtype"],
           "steps": args.steps, "warmup": args.warmup, "frac": args.frac, "ms_median": res_ms, "ms_min": res_min,
           "ms_p10": res_p10, "ms_p90": res_p90, "legs": legs,
           "scratch_bytes": {"split": 16 * 4096 * tiles, "merge": 8 * 4096 * tiles},
           "peak_tb_s_assumed": PEAK_TB_S, "device": torch.cuda.get_device_name(0),
           "library": capi.load_library().wc_version().decode()}
    line = json.dumps(res)
    print(line)
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
