#!/usr/bin/env python3
"""Cost and gain of the pointwise (max-abs) error bound, one library build.

On a bench_workloads shape (default C2: 1024 x 64^3 fp64), device buffers, the
context's own stream, host clock around call + wc_synchronize, alternating, for
each L of --levels (each unit at wc_levels_for(dims, L)):
    maxerr_L          wc_forward_levels_maxerr, every unit's bound = --frac times its max|x|
    leveltol_L        wc_forward_levels_tol at --rms-frac times each unit's RMS
    levels_thresh_L   wc_forward_levels with an explicit threshold: the same dense
                      staging, level passes and emit with one threshold
    baseline_L        the search a caller composes from the other entry points: one
                      wc_decompose_levels, then per pass 15 candidates of a mask in
                      torch + wc_inverse_flat_levels + a max reduction in torch, and
                      one read-back per pass; then err(b*): 46 probes.  The
                      thresholds it finds are asserted equal to the mode's.  It stops
                      at the thresholds: writing the payloads takes a forward more.
                      Units of one size only (the mask and the reduction are batched
                      by reshaping).
Medians of --steps calls each after --warmup, then one profiled pass per leg for
the stage times (WC_STAGE_TOL of maxerr_L: the three probe passes, the pick and the
mask pass; a second profiled pass of leveltol_L gives the mask pass's share to
subtract).  Per L also the gain of verifying: kept pairs and RMSE (root mean
square over units) at the found thresholds against the analytic threshold
E / (7 L + 1) per unit, the latter applied by the mask + wc_inverse_flat_levels
route (wc_forward_levels takes one threshold for all units; the kept set and the
reconstruction are the same).

    python tools/bench_maxerr.py --steps 20 --warmup 3 --out profiles/r23/maxerr.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frac", type=float, default=0.01, help="each unit's bound as a fraction of its max|x|")
    ap.add_argument("--rms-frac", type=float, default=0.01, help="the leveltol legs' tolerance as a fraction of the RMS")
    ap.add_argument("--thresh", type=float, default=0.35, help="the explicit threshold of the levels_thresh legs")
    ap.add_argument("--levels", default="1,3")
    ap.add_argument("--baseline-steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    Ls = tuple(int(x) for x in args.levels.split(","))

    import numpy as np
    import torch
    import wcamd
    import bench_workloads as bw
    capi = wcamd.capi

    if not torch.cuda.is_available():
        raise SystemExit("bench_maxerr.py needs a HIP device")
    dev = torch.device("cuda", 0)
    wl = bw.WORKLOADS[args.workload]
    units_py = wl["units"]()
    cells, offsets, extent = bw.synth_cells(torch, dev, units_py, wl["dtype"])
    units, n, _ = bw.units_array(capi, units_py, offsets)
    dtype = capi.WC_F64 if wl["dtype"] == "f64" else capi.WC_F32
    ncells = sum(u.cells for u in units_py)
    sizes = [units[i].nx * units[i].ny * units[i].nz for i in range(n)]
    per = sizes[0]
    uniform = all(s == per for s in sizes) and all(units[i].cell_offset == i * per for i in range(n)) and extent == n * per
    view = cells.view(n, per) if uniform else None
    if uniform:
        amax = view.abs().amax(dim=1).double().cpu().numpy()
        rms = view.double().pow(2).mean(dim=1).sqrt().cpu().numpy()
    else:
        sl = [cells[units[i].cell_offset:units[i].cell_offset + sizes[i]].double() for i in range(n)]
        amax = np.array([float(s.abs().max().item()) if s.numel() else 0.0 for s in sl])
        rms = np.array([float(s.pow(2).mean().sqrt().item()) if s.numel() else 0.0 for s in sl])
    E = args.frac * amax
    tol = args.rms_frac * rms
    lv = {L: [capi.levels_for(units[i].nx, units[i].ny, units[i].nz, L) for i in range(n)] for L in Ls}
    cap = capi.payload_bound(units, n)
    pay = torch.empty(cap, dtype=torch.uint8, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    kept = torch.zeros(n, dtype=torch.int32, device=dev)
    thresh = torch.zeros(n, dtype=torch.float32, device=dev)
    thresh4 = torch.zeros(n * capi.WC_MAX_LEVELS, dtype=torch.float32, device=dev)
    err = torch.zeros(n, dtype=torch.float64, device=dev)
    bound = torch.zeros(n, dtype=torch.float64, device=dev)
    flat = torch.empty(max(extent, 1), dtype=torch.float32, device=dev)
    masked = torch.empty_like(flat)
    regen = torch.empty(max(extent, 1), dtype=torch.float32, device=dev)
    rmse = torch.zeros(n, dtype=torch.float64, device=dev)
    E_d = torch.from_numpy(E).to(dev)
    torch.cuda.synchronize()
    ctx = capi.Context(0)
    outs = (pay.data_ptr(), cap, off.data_ptr(), kept.data_ptr())
    flt_max = float(np.finfo(np.float32).max)

    def thr_of(b):  # int64 tensor of bins -> fp32 thresholds
        bits = ((b << 19) - 1).clamp(min=0).to(torch.int32).view(torch.float32)
        return torch.where(b == 0, torch.zeros_like(bits), torch.where(b >= 0xFF0, torch.full_like(bits, flt_max), bits))

    def probe(L, b):
        """err(b[u]) of every unit by the caller's route: mask, wc_inverse_flat_levels, max in torch."""
        t = thr_of(b).view(n, 1)
        f = flat.view(n, per)
        torch.where(f.abs() > t, f, torch.zeros((), dtype=torch.float32, device=dev), out=masked.view(n, per))
        torch.cuda.current_stream().synchronize()  # torch's stream -> the context's
        ctx.inverse_flat_levels(masked.data_ptr(), units, n, lv[L], regen.data_ptr())
        ctx.synchronize()
        d = (view.double() - regen.view(n, per).double()).abs()
        return torch.nan_to_num(d, nan=0.0, posinf=math.inf).amax(dim=1)

    def baseline(L):
        def run():
            ctx.decompose_levels(cells.data_ptr(), dtype, units, n, lv[L], flat.data_ptr())
            ctx.synchronize()
            lo = torch.zeros(n, dtype=torch.int64, device=dev)
            for stride in (256, 16, 1):
                errs = torch.stack([probe(L, lo + i * stride) for i in range(1, 16)], dim=1)  # [n, 15]
                ok = (errs <= E_d.view(n, 1)).cpu().numpy()  # the pass's read-back
                j = np.array([int(np.argmin(r)) if not r.all() else 15 for r in ok])
                lo = lo + torch.from_numpy(j * stride).to(dev)
            run.err = probe(L, lo)  # the 46th probe: err(b*)
            run.thresh = thr_of(lo)
        return run

    fwd = {}
    for L in Ls:
        fwd[f"maxerr_L{L}"] = (lambda L=L: ctx.forward_levels_maxerr(cells.data_ptr(), dtype, units, n, lv[L], E, *outs,
                                                                     thresh.data_ptr(), err.data_ptr()))
        fwd[f"leveltol_L{L}"] = (lambda L=L: ctx.forward_levels_tol(cells.data_ptr(), dtype, units, n, lv[L], tol, *outs,
                                                                    thresh4.data_ptr(), bound.data_ptr()))
        fwd[f"levels_thresh_L{L}"] = (lambda L=L: ctx.forward_levels(cells.data_ptr(), dtype, units, n, lv[L], 0.0,
                                                                     args.thresh, *outs))

    def timed(fn):
        ctx.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    times = {k: [] for k in fwd}
    for step in range(args.warmup + args.steps):
        for name, fn in fwd.items():  # alternating: drift hits every variant alike
            dt = timed(fn)
            if step >= args.warmup:
                times[name].append(dt)

    stages, legs, gain = {}, {}, {}
    for name, fn in fwd.items():
        ctx.profile_enable(True)
        fn()
        ctx.synchronize()
        stages[name] = {k: round(v[0], 4) for k, v in ctx.profile_read().items()}
        ctx.profile_enable(False)
        L = int(name[-1])
        ctx.inverse_levels(pay.data_ptr(), off.data_ptr(), units, n, lv[L], regen.data_ptr())
        ctx.rmse(cells.data_ptr(), dtype, regen.data_ptr(), units, n, rmse.data_ptr())
        ctx.maxerr(cells.data_ptr(), dtype, regen.data_ptr(), units, n, bound.data_ptr())
        ctx.synchronize()
        k = int(kept.sum().item())
        legs[name] = {"kept_pairs": k, "payload_bytes": 20 * n + 8 * k,
                      "rmse": math.sqrt(float((rmse * rmse).mean().item())),
                      "max_err_over_E": float((bound / E_d).max().item())}
        if name.startswith("maxerr"):
            legs[name]["err_equals_wc_maxerr_units"] = int((bound == err).sum().item())
            legs[name]["units_at_b0"] = int((thresh == 0).sum().item())
            found = thresh.clone()
            if uniform:
                # the gain of verifying: the analytic threshold E / (7 L + 1) per unit by the caller's route
                ctx.decompose_levels(cells.data_ptr(), dtype, units, n, lv[L], flat.data_ptr())
                ctx.synchronize()
                ta = (E_d / (7 * L + 1)).float().view(n, 1)
                f = flat.view(n, per)
                keep_a = f.abs() > ta
                torch.where(keep_a, f, torch.zeros((), dtype=torch.float32, device=dev), out=masked.view(n, per))
                torch.cuda.synchronize()
                ctx.inverse_flat_levels(masked.data_ptr(), units, n, lv[L], regen.data_ptr())
                ctx.rmse(cells.data_ptr(), dtype, regen.data_ptr(), units, n, rmse.data_ptr())
                ctx.maxerr(cells.data_ptr(), dtype, regen.data_ptr(), units, n, bound.data_ptr())
                ctx.synchronize()
                ka = int(keep_a.sum().item())
                gain[f"L{L}"] = {"kept_pairs_found": k, "kept_pairs_analytic": ka, "pairs_ratio": round(ka / max(k, 1), 3),
                                 "rmse_found": legs[name]["rmse"],
                                 "rmse_analytic": math.sqrt(float((rmse * rmse).mean().item())),
                                 "max_err_over_E_analytic": float((bound / E_d).max().item()),
                                 "median_thresh_found_over_analytic": float((found.double().view(n, 1) / ta.double()).median().item())}
                # the caller's search, timed on its own (it is two orders slower: fewer steps)
                run = baseline(L)
                bt = [timed(run) for _ in range(1 + args.baseline_steps)][1:]
                times[f"baseline_L{L}"] = bt
                legs[f"baseline_L{L}"] = {"thresholds_equal_units": int((run.thresh == found).sum().item()),
                                          "errs_equal_units": int((run.err == err).sum().item())}
                assert legs[f"baseline_L{L}"]["thresholds_equal_units"] == n

    med = {k: statistics.median(v) for k, v in times.items()}
    probes = {}
    for L in Ls:
        mask_ms = stages[f"leveltol_L{L}"].get("tol", 0.0)  # bins + pick + mask: an upper bound of the mask pass
        probes[f"L{L}"] = {"tol_stage_ms": stages[f"maxerr_L{L}"].get("tol", 0.0), "leveltol_tol_stage_ms": mask_ms}
    res = {
        "bench": "maxerr", "workload": args.workload, "units": n, "cells": ncells, "dtype": wl["dtype"],
        "steps": args.steps, "warmup": args.warmup, "frac": args.frac, "rms_frac": args.rms_frac, "thresh": args.thresh,
        "ms_median": {k: round(v, 4) for k, v in med.items()},
        "ms_min": {k: round(min(v), 4) for k, v in times.items()},
        "ms_p90": {k: round(sorted(v)[int(0.9 * (len(v) - 1))], 4) for k, v in times.items()},
        "legs": legs, "stage_ms": stages, "probe_stage": probes, "gain_of_verifying": gain,
        "maxerr_over_baseline": {f"L{L}": round(med[f"maxerr_L{L}"] / med[f"baseline_L{L}"], 4)
                                 for L in Ls if f"baseline_L{L}" in med},
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
