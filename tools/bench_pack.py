#!/usr/bin/env python3
"""Cost of the packed payloads (wc_pack / wc_unpack) beside the forward and the inverse, one library build.

On a bench_workloads shape (default C2: 1024 x 64^3 fp64) at the workload's keep,
device buffers, the context's own stream, host clock around call + wc_synchronize,
alternating:
    forward          wc_forward, which writes the payloads the other legs read
    inverse          wc_inverse of them
    pack{2,3,4}      wc_pack at V = 2, 3, 4 value bytes
    unpack{2,3,4}    wc_unpack of each
Medians of --steps calls each after --warmup, then one profiled pass per leg
(WC_STAGE_PACK), the packed bytes per pair, and a check that unpack{4} gives the
forward's bytes back.

Then on the host, for the first --host-units units (the C3-like question: what
reaches xz): xz preset 6 of the standard payloads against xz of the packed units
at each V, bytes and seconds on one thread; wc_pack_host against --threads threads
of wc_pack_unit (the plain-C++ rule) on the same units.

Estimate from bytes, written before the first run: wc_pack reads the pairs twice
(the widths pass, then the body) and writes the packed bytes once; wc_unpack reads
the packed bytes and writes the pairs.  C2 at keep 0.999 has 81.3 M pairs, 0.651
GB; a second read that comes from HBM too is 1.30 GB read + about 0.35 GB written
at V = 4, 0.3 ms at 5 TB/s: a few tenths of a millisecond, an expectation and not
a bar.

    python tools/bench_pack.py --steps 30 --warmup 5 --out profiles/r14/pack.json
"""
from __future__ import annotations

import argparse
import ctypes
import json
import lzma
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-units", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
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
        raise SystemExit("bench_pack.py needs a HIP device")
    dev = torch.device("cuda", 0)
    wl = bw.WORKLOADS[args.workload]
    units_py = wl["units"]()
    cells, offsets, extent = bw.synth_cells(torch, dev, units_py, wl["dtype"])
    units, n, _ = bw.units_array(capi, units_py, offsets)
    dtype = capi.WC_F64 if wl["dtype"] == "f64" else capi.WC_F32
    keep = float(np.float32(wl["keep"]))
    cap = capi.payload_bound(units, n)
    pay = torch.empty(cap, dtype=torch.uint8, device=dev)
    back = torch.empty(cap, dtype=torch.uint8, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    off2 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    kept = torch.zeros(n, dtype=torch.int32, device=dev)
    kept2 = torch.zeros(n, dtype=torch.int32, device=dev)
    regen = torch.empty(max(extent, 1), dtype=torch.float32, device=dev)
    VS = (2, 3, 4)
    pcap = {V: capi.packed_bound(units, n, V) for V in VS}
    packed = torch.empty(max(pcap.values()), dtype=torch.uint8, device=dev)
    poff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    pbytes = torch.zeros(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx = capi.Context(0)

    def forward():
        ctx.forward(cells.data_ptr(), dtype, units, n, keep, pay.data_ptr(), cap, off.data_ptr(), kept.data_ptr())

    def inverse():
        ctx.inverse(pay.data_ptr(), off.data_ptr(), units, n, regen.data_ptr())

    def pack(V):
        return lambda: ctx.pack(pay.data_ptr(), off.data_ptr(), units, n, V, packed.data_ptr(), pcap[V], poff.data_ptr(),
                                pbytes.data_ptr())

    def unpack(V):
        return lambda: ctx.unpack(packed.data_ptr(), poff.data_ptr(), pcap[V], units, n, back.data_ptr(), cap,
                                  off2.data_ptr(), kept2.data_ptr())

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

    forward()
    ctx.synchronize()
    pairs = int(kept.sum().item())
    legs = {"forward": forward, "inverse": inverse}
    for V in VS:  # unpack{V} reads what pack{V} just wrote: the pair stays together in the rotation
        legs[f"pack{V}"] = pack(V)
        legs[f"unpack{V}"] = unpack(V)
    times = {k: [] for k in legs}
    for step in range(args.warmup + args.steps):
        for name, fn in legs.items():
            dt = timed(fn)
            if step >= args.warmup:
                times[name].append(dt)
    stages = {name: profiled(fn) for name, fn in legs.items()}
    packed_bytes = {}
    for V in VS:
        pack(V)()
        unpack(V)()
        ctx.synchronize()
        packed_bytes[V] = int(pbytes.sum().item())
        if V == 4:
            ok = bool(torch.equal(kept, kept2)) and bool(torch.equal(off, off2))
            h_pay, h_back, h_off, h_kept = pay.cpu().numpy(), back.cpu().numpy(), off.cpu().numpy(), kept.cpu().numpy()
            for i in range(0, n, max(1, n // 64)):
                o, m = int(h_off[i]), 20 + 8 * int(h_kept[i])
                ok = ok and h_pay[o:o + m].tobytes() == h_back[o:o + m].tobytes()
            if not ok:
                raise SystemExit("unpack(pack(p), 4) is not p")

    # ---- the host side, on the first units ---------------------------------------------------
    m = min(args.host_units, n)
    h_pay, h_off, h_kept = pay.cpu().numpy(), off.cpu().numpy().astype(np.uint64), kept.cpu().numpy()
    std = [h_pay[int(h_off[i]):int(h_off[i]) + 20 + 8 * int(h_kept[i])].tobytes() for i in range(m)]
    sub_units, _, _ = capi.make_units([(units[i].nx, units[i].ny, units[i].nz) for i in range(m)])

    def xz(blobs):
        t0 = time.perf_counter()
        size = sum(len(lzma.compress(b, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64, preset=6)) for b in blobs)
        return size, time.perf_counter() - t0

    L = capi.load_library()
    host = {"units": m, "pairs": int(h_kept[:m].sum()), "standard_bytes": sum(len(s) for s in std)}
    host["standard_xz6_bytes"], host["standard_xz6_s"] = xz(std)
    span = h_pay[:int(h_off[m - 1]) + 20 + 8 * int(h_kept[m - 1])]
    for V in VS:
        ctx.pack_host(span, h_off[:m], sub_units, m, V)  # buffers grown, descriptors uploaded
        t0 = time.perf_counter()
        pk, po, pb = ctx.pack_host(span, h_off[:m], sub_units, m, V)
        t_dev = time.perf_counter() - t0
        blobs = [pk[int(po[i]):int(po[i]) + int(pb[i])].tobytes() for i in range(m)]
        outs = [np.empty(len(b) + 8, np.uint8) for b in blobs]
        srcs = [np.frombuffer(s, np.uint8) for s in std]

        def one(i, V=V):
            w = ctypes.c_size_t()
            rc = L.wc_pack_unit(srcs[i].ctypes.data, srcs[i].size, V, outs[i].ctypes.data, outs[i].size, ctypes.byref(w))
            assert rc == 0 and w.value == len(blobs[i])

        with ThreadPoolExecutor(args.threads) as pool:
            t0 = time.perf_counter()
            list(pool.map(one, range(m)))
            t_cpu = time.perf_counter() - t0
        assert all(outs[i][:len(blobs[i])].tobytes() == blobs[i] for i in range(m))
        size, secs = xz(blobs)
        host[f"V{V}"] = {"packed_bytes": sum(len(b) for b in blobs), "xz6_bytes": size, "xz6_s": round(secs, 4),
                         "pack_host_ms": round(t_dev * 1e3, 3), f"pack_unit_{args.threads}_threads_ms": round(t_cpu * 1e3, 3)}
    host["standard_xz6_s"] = round(host["standard_xz6_s"], 4)

    res = {
        "bench": "pack", "workload": args.workload, "units": n, "dtype": wl["dtype"], "keep": keep, "pairs": pairs,
        "payload_bytes": 20 * n + 8 * pairs, "steps": args.steps, "warmup": args.warmup,
        "ms_median": {k: round(statistics.median(v), 4) for k, v in times.items()},
        "ms_min": {k: round(min(v), 4) for k, v in times.items()},
        "ms_p90": {k: round(sorted(v)[int(0.9 * (len(v) - 1))], 4) for k, v in times.items()},
        "stage_ms": stages,
        "packed_bytes": {f"V{V}": packed_bytes[V] for V in VS},
        "packed_bytes_per_pair": {f"V{V}": round(packed_bytes[V] / max(pairs, 1), 4) for V in VS},
        "host": host,
        "device": torch.cuda.get_device_name(0), "library": L.wc_version().decode(),
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
