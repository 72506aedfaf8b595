#!/usr/bin/env python3
"""Reading packed payloads: the direct decoders against wc_unpack + the standard decoders, one library build.

On a bench_workloads shape (default C2: 1024 x 64^3 fp64) at the workload's keep,
payloads with one level (wc_forward) and with three (wc_forward_levels), packed at
V = 2, 3, 4 (wc_pack).  Device buffers, the context's own stream, host clock
around call(s) + wc_synchronize.  For every (L, V), in one process, interleaved in
one rotation:
    full      wc_inverse_packed                    | wc_unpack + wc_inverse_levels
    coarse    wc_inverse_packed_coarse, r = 1      | wc_unpack + wc_inverse_coarse
    slab      wc_inverse_packed_region, x < 8      | wc_unpack + wc_inverse_region
    block     wc_inverse_packed_region, one 8^3    | wc_unpack + wc_inverse_region
The right-hand calls are the unchanged entry points.  Medians of --steps calls
after --warmup, with min, p10 and p90 as the spread; `verdict` says per leg
whether the direct call is not slower beyond the spread (its median at most the
two-call median, or the two [p10, p90] ranges overlap).  Every direct result is
compared with the two-call result once, bit for bit.

Device memory: what a context allocates for each path on a fresh context (free
device memory before and after the first call), and the standard payload buffer
(wc_payload_bound) the two-call path needs from the caller on top of it.

Estimate from bytes, written before the first run: the two-call path reads the
packed bytes, writes 8 B per pair and reads them back; the direct path reads the
packed bytes once.  C2 at keep 0.999 has about 81 M pairs: 0.65 GB written and
0.65 GB read again that the direct path does not move, 0.25-0.3 ms at 5 TB/s.
An expectation, not a bar.

    python tools/bench_packed_decode.py --steps 30 --warmup 5 --out profiles/r17/packed_decode.json
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
        raise SystemExit("bench_packed_decode.py needs a HIP device")
    dev = torch.device("cuda", 0)
    wl = bw.WORKLOADS[args.workload]
    units_py = wl["units"]()
    cells, offsets, extent = bw.synth_cells(torch, dev, units_py, wl["dtype"])
    units, n, _ = bw.units_array(capi, units_py, offsets)
    dtype = capi.WC_F64 if wl["dtype"] == "f64" else capi.WC_F32
    keep = float(np.float32(wl["keep"]))
    cap = capi.payload_bound(units, n)
    VS, LS = (2, 3, 4), (1, 3)
    pay = torch.empty(cap, dtype=torch.uint8, device=dev)       # the forward's payloads, then wc_unpack's scratch
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    kept = torch.zeros(n, dtype=torch.int32, device=dev)
    pcap = {V: capi.packed_bound(units, n, V) for V in VS}
    pbytes = torch.zeros(n, dtype=torch.int64, device=dev)
    ctx = capi.Context(0)

    # the derived units of the three reduced calls
    dims = [(u.W, u.H, u.D) for u in units_py]
    coarse_units, coarse_ext = capi.coarse_units(units, n, 1)
    slab = [(0, 0, 0, 8, H, D) for W, H, D in dims]
    block = [(W - 8, H - 8, D - 8, 8, 8, 8) for W, H, D in dims]
    slab_units, slab_ext = capi.region_units(units, n, slab, 0)
    block_units, block_ext = capi.region_units(units, n, block, 0)
    out = {k: torch.empty(max(e, 1), dtype=torch.float32, device=dev)
           for k, e in (("full", extent), ("coarse", coarse_ext), ("slab", slab_ext), ("block", block_ext))}
    ref = {k: torch.empty_like(v) for k, v in out.items()}

    # the packed units of every (L, V), kept side by side
    packed, poff, pairs, packed_bytes = {}, {}, {}, {}
    for L in LS:
        if L == 1:
            ctx.forward(cells.data_ptr(), dtype, units, n, keep, pay.data_ptr(), cap, off.data_ptr(), kept.data_ptr())
        else:
            ctx.forward_levels(cells.data_ptr(), dtype, units, n, L, keep, None, pay.data_ptr(), cap, off.data_ptr(),
                               kept.data_ptr())
        ctx.synchronize()
        pairs[L] = int(kept.sum().item())
        for V in VS:
            packed[L, V] = torch.empty(pcap[V], dtype=torch.uint8, device=dev)
            poff[L, V] = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            ctx.pack(pay.data_ptr(), off.data_ptr(), units, n, V, packed[L, V].data_ptr(), pcap[V],
                     poff[L, V].data_ptr(), pbytes.data_ptr())
            ctx.synchronize()
            packed_bytes[L, V] = int(pbytes.sum().item())
    del cells
    off2 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    kept2 = torch.zeros(n, dtype=torch.int32, device=dev)

    def unpack(c, L, V):
        c.unpack(packed[L, V].data_ptr(), poff[L, V].data_ptr(), pcap[V], units, n, pay.data_ptr(), cap, off2.data_ptr(),
                 kept2.data_ptr())

    def direct(c, mode, L, V, dst):
        a = (packed[L, V].data_ptr(), poff[L, V].data_ptr(), pcap[V], units, n, L)
        if mode == "full":
            c.inverse_packed(*a, dst["full"].data_ptr())
        elif mode == "coarse":
            c.inverse_packed_coarse(*a, 1, coarse_units, dst["coarse"].data_ptr())
        elif mode == "slab":
            c.inverse_packed_region(*a, 0, slab, slab_units, dst["slab"].data_ptr())
        else:
            c.inverse_packed_region(*a, 0, block, block_units, dst["block"].data_ptr())

    def two_calls(c, mode, L, V, dst):
        unpack(c, L, V)
        a = (pay.data_ptr(), off2.data_ptr(), units, n, L)
        if mode == "full":
            c.inverse_levels(*a, dst["full"].data_ptr())
        elif mode == "coarse":
            c.inverse_coarse(*a, 1, coarse_units, dst["coarse"].data_ptr())
        elif mode == "slab":
            c.inverse_region(*a, 0, slab, slab_units, dst["slab"].data_ptr())
        else:
            c.inverse_region(*a, 0, block, block_units, dst["block"].data_ptr())

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    MODES = ("full", "coarse", "slab", "block")
    legs = {}
    for L in LS:
        for V in VS:
            for mode in MODES:
                legs[f"L{L}/V{V}/{mode}/direct"] = (lambda m=mode, l=L, v=V: direct(ctx, m, l, v, out))
                legs[f"L{L}/V{V}/{mode}/unpack+decode"] = (lambda m=mode, l=L, v=V: two_calls(ctx, m, l, v, ref))
    # the results agree, bit for bit
    for L in LS:
        for V in VS:
            for mode in MODES:
                out[mode].fill_(-1.0)
                ref[mode].fill_(-2.0)
                torch.cuda.synchronize()
                direct(ctx, mode, L, V, out)
                two_calls(ctx, mode, L, V, ref)
                ctx.synchronize()
                if not torch.equal(out[mode].view(torch.int32), ref[mode].view(torch.int32)):
                    raise SystemExit(f"L{L} V{V} {mode}: the direct call and unpack + decode disagree")
    times = {k: [] for k in legs}
    for step in range(args.warmup + args.steps):
        for name, fn in legs.items():
            dt = timed(fn)
            if step >= args.warmup:
                times[name].append(dt)
    unpack_ms = {}
    for L in LS:
        for V in VS:
            unpack_ms[f"L{L}/V{V}"] = round(statistics.median(timed(lambda: unpack(ctx, L, V)) for _ in range(args.steps)), 4)

    def stat(v):
        s = sorted(v)
        return {"median": round(statistics.median(s), 4), "min": round(s[0], 4), "p10": round(s[int(0.1 * (len(s) - 1))], 4),
                "p90": round(s[int(0.9 * (len(s) - 1))], 4)}

    ms = {k: stat(v) for k, v in times.items()}
    verdict = {}
    for k in ms:
        if k.endswith("/direct"):
            d, t = ms[k], ms[k[:-len("direct")] + "unpack+decode"]
            verdict[k[:-len("/direct")]] = {
                "direct_over_two_calls": round(d["median"] / t["median"], 4),
                "not_slower_beyond_spread": bool(d["median"] <= t["median"] or d["p10"] <= t["p90"]),
            }
    ctx.close()

    # ---- device memory a fresh context allocates for each path (bytes of free memory that went away)
    def allocated(fn):
        torch.cuda.synchronize()
        c = capi.Context(0)
        c.synchronize()
        before = torch.cuda.mem_get_info()[0]
        fn(c)
        c.synchronize()
        after = torch.cuda.mem_get_info()[0]
        c.close()
        return int(before - after)

    L, V = 1, 3
    memory = {"wc_payload_bound_bytes_the_two_call_path_needs_from_the_caller": int(cap)}
    for mode in MODES:
        memory[mode] = {"direct_context_bytes": allocated(lambda c, m=mode: direct(c, m, L, V, out)),
                        "unpack+decode_context_bytes": allocated(lambda c, m=mode: two_calls(c, m, L, V, ref))}
        memory[mode]["unpack+decode_total_bytes"] = memory[mode]["unpack+decode_context_bytes"] + int(cap)
        memory[mode]["output_bytes"] = int(out[mode].numel() * 4)

    res = {
        "bench": "packed_decode", "workload": args.workload, "units": n, "dtype": wl["dtype"], "keep": keep,
        "pairs": {f"L{L}": pairs[L] for L in LS}, "steps": args.steps, "warmup": args.warmup,
        "packed_bytes": {f"L{L}/V{V}": packed_bytes[L, V] for L in LS for V in VS},
        "ms": ms, "unpack_alone_ms_median": unpack_ms, "verdict": verdict, "memory": memory,
        "device": torch.cuda.get_device_name(0), "library": capi.load_library().wc_version().decode(),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        p = Path(args.out)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(line + "\n")


if __name__ == "__main__":
    main()
