"""GPU: the RMSE-tolerance mode (include/wavelet_amd.h wc_forward_tol /
wc_forward_emit_tol / wc_forward_tol_host, the CLI's `rmse=`) against the
numpy restatement of the selection rule (tol_rule.py) on the oracle's
coefficients.

Bar: per unit, the device's threshold and model bound equal the rule's bit for
bit; the payload bytes equal the reference's mask + RLE + serialize applied
with that threshold (oracle.compress_payload_thresh); kept counts and slot
offsets follow; the solo and split binning paths (WC_OPT_TOL_SOLO_TILES at its
default and at 1) give identical outputs; the actual RMSE of the round trip is
within tol * (1 + MARGIN) for tol >= 1e-3 (tol_rule.py derives the margin)."""
import math
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_cli import CLI, digit_free_dir
from tol_rule import MARGIN, field, same_bits, tol_rule
from wavelet_compression_amd.capi import WC_OPT_HOST_CHUNK, WC_OPT_TOL_SOLO_TILES

pytestmark = pytest.mark.gpu

# generic transform (D % 8 != 0); fast path: half a flat tile, exactly one, a
# ragged second one, the widest fast tile (two tiles); no cells; a constant box
DIMS = [(2, 2, 2), (4, 2, 6), (16, 16, 8), (16, 16, 16), (16, 16, 24), (32, 32, 8), (0, 4, 4), (16, 16, 16),
        (4, 2, 6), (16, 16, 24), (32, 32, 8), (2, 2, 2)]
KINDS = [0, 1, 2, 0, 2, 0, 0, 3, 2, 1, 2, 1]
TOL_A = [1e-2, 1.0, 1e-3, 0.1, 1e-2, 0.1, 1.0, 0.0, math.inf, 1.0, 1e-3, 0.0]
TOL_B = [0.0, 1e-3, 1.0, math.inf, 0.1, 1e-2, 0.0, 1.0, 1e-2, 1e-3, math.inf, 0.1]


def make_batch(wc, dtype):
    boxes = [field(k, *d, seed=100 + i) if d[0] else np.zeros((d[2], d[1], 0), np.float32)
             for i, (d, k) in enumerate(zip(DIMS, KINDS))]
    units, n, extent = wc.capi.make_units(DIMS)
    cells = np.zeros(max(extent, 1), dtype)
    for i, b in enumerate(boxes):
        o = units[i].cell_offset
        cells[o:o + b.size] = b.ravel().astype(dtype)
    return boxes, units, n, extent, cells


@pytest.fixture(scope="module")
def expect(oracle):
    """The rule on the oracle's coefficients, once per (unit, tolerance):
    (thresh, bound, payload bytes, kept)."""
    cache = {}

    def get(i, box, tol):
        key = (i, tol)
        if key not in cache:
            D, H, W = box.shape
            if box.size == 0:
                t, b = tol_rule(np.zeros(4096, np.uint64), 0, tol)
                cache[key] = (t, b, np.array([W, H, D, 0, 0], "<i4").tobytes(), 0)
            else:
                flat = oracle.wavelet_decompose(box)
                t, b = tol_rule(oracle.magnitude_hist(flat), flat.size, tol)
                p = oracle.compress_payload_thresh(box, t)
                cache[key] = (t, b, p, int(np.frombuffer(p[16:20], "<i4")[0]))
        return cache[key]
    return get


class Dev:
    """Device buffers of one batch."""

    def __init__(self, wc, cells, units, n):
        import torch
        dev = torch.device("cuda", 0)
        self.wc, self.units, self.n = wc, units, n
        self.dtype = wc.capi.WC_F64 if cells.dtype == np.float64 else wc.capi.WC_F32
        self.cells = torch.from_numpy(cells).to(dev)
        self.cap = wc.capi.payload_bound(units, n)
        self.pay = torch.zeros(self.cap, dtype=torch.uint8, device=dev)
        self.off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        self.kept = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.thresh = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
        self.bound = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()  # the fills run on torch's stream, the context on its own

    def out_args(self):
        return (self.pay.data_ptr(), self.cap, self.off.data_ptr(), self.kept.data_ptr(), self.thresh.data_ptr(),
                self.bound.data_ptr())

    def read(self):
        pay = self.pay.cpu().numpy()
        off = self.off.cpu().numpy().view(np.uint64)
        kept = self.kept.cpu().numpy().view(np.uint32)
        payloads = [self.wc.capi.unit_payload(pay, off, kept, i) for i in range(self.n)]
        return payloads, kept.copy(), off.copy(), self.thresh.cpu().numpy(), self.bound.cpu().numpy()


def forward_tol(wc, ctx, cells, units, n, tol, staged=False):
    d = Dev(wc, cells, units, n)
    if staged:
        ctx.forward_stage(d.cells.data_ptr(), d.dtype, units, n, None)
        ctx.forward_emit_tol(units, n, tol, *d.out_args())
    else:
        ctx.forward_tol(d.cells.data_ptr(), d.dtype, units, n, tol, *d.out_args())
    ctx.synchronize()
    return d.read()


def check_outputs(out, boxes, units, tols, expect):
    payloads, kept, off, thresh, bound = out
    n = len(boxes)
    slot = 4
    for i, b in enumerate(boxes):
        t, bd, p, k = expect(i, b, tols[i])
        what = (i, DIMS[i], tols[i])
        assert same_bits(float(thresh[i]), t, np.float32), (what, float(thresh[i]), t)
        assert same_bits(float(bound[i]), bd), (what, float(bound[i]), bd)
        assert bound[i] <= tols[i]
        assert int(kept[i]) == k, what
        assert payloads[i] == p, what
        assert int(off[i]) == slot, what  # the slot rule of wc_forward
        slot += 24 + 8 * b.size
    assert int(off[n]) == int(off[n - 1]) + 20 + 8 * int(kept[n - 1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_forward_tol_bit_exact_solo_and_split(wc, ctx, expect, dtype):
    boxes, units, n, extent, cells = make_batch(wc, dtype)
    assert ctx.get_option(WC_OPT_TOL_SOLO_TILES) >= 63
    solo = forward_tol(wc, ctx, cells, units, n, TOL_A)
    check_outputs(solo, boxes, units, TOL_A, expect)
    ctx.set_option(WC_OPT_TOL_SOLO_TILES, 1)  # every unit of two tiles (16x16x24, 32x32x8) is split
    try:
        split = forward_tol(wc, ctx, cells, units, n, TOL_A)
    finally:
        ctx.set_option(WC_OPT_TOL_SOLO_TILES, 64)
    check_outputs(split, boxes, units, TOL_A, expect)
    assert solo[0] == split[0]
    for a, b in zip(solo[1:], split[1:]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("solo_tiles", [64, 1])
def test_stage_then_emit_tol_twice(wc, ctx, expect, solo_tiles):
    """wc_forward_stage + wc_forward_emit_tol gives wc_forward_tol's bytes, and a
    second emit with other tolerances reuses the staged coefficients."""
    boxes, units, n, extent, cells = make_batch(wc, np.float64)
    ctx.set_option(WC_OPT_TOL_SOLO_TILES, solo_tiles)
    try:
        direct = forward_tol(wc, ctx, cells, units, n, TOL_A)
        d = Dev(wc, cells, units, n)
        ctx.forward_stage(d.cells.data_ptr(), d.dtype, units, n, None)
        ctx.forward_emit_tol(units, n, TOL_A, *d.out_args())
        ctx.synchronize()
        first = d.read()
        ctx.forward_emit_tol(units, n, TOL_B, *d.out_args())
        ctx.synchronize()
        second = d.read()
        # nullable outputs: no thresholds or bounds asked for
        ctx.forward_emit_tol(units, n, TOL_A, d.pay.data_ptr(), d.cap, d.off.data_ptr(), d.kept.data_ptr())
        ctx.synchronize()
        third = d.read()
    finally:
        ctx.set_option(WC_OPT_TOL_SOLO_TILES, 64)
    assert first[0] == direct[0] and first[1].tobytes() == direct[1].tobytes()
    check_outputs(first, boxes, units, TOL_A, expect)
    check_outputs(second, boxes, units, TOL_B, expect)
    assert third[0] == first[0] and third[3].tobytes() == second[3].tobytes()  # thresholds untouched


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_forward_tol_host(wc, ctx, oracle, expect, dtype):
    """wc_forward_tol_host: the device call's payloads, packed; its rmse output
    is the RMSE of wc_inverse_host of those payloads (within 1e-12, the fused
    RMSE's tolerance) and within the tolerance; also over several unit runs."""
    boxes, units, n, extent, cells = make_batch(wc, dtype)
    want = forward_tol(wc, ctx, cells, units, n, TOL_A)
    outs = [ctx.forward_tol_host(cells, units, n, TOL_A)]
    ctx.set_option(WC_OPT_HOST_CHUNK, 3000)
    try:
        outs.append(ctx.forward_tol_host(cells, units, n, TOL_A))
    finally:
        ctx.set_option(WC_OPT_HOST_CHUNK, 1 << 25)
    for payload, offs, kept, thresh, bound, rmse in outs:
        assert kept.tobytes() == want[1].tobytes()
        assert thresh.tobytes() == want[3].tobytes() and bound.tobytes() == want[4].tobytes()
        pos = 4
        for i in range(n):
            assert int(offs[i]) == pos, i  # packed as wc_forward_host: 24 + 8 * kept apart
            assert wc.capi.unit_payload(payload, offs, kept, i) == want[0][i], i
            pos += 24 + 8 * int(kept[i])
        regen = ctx.inverse_host(payload, offs[:n], units, n, extent)
        ref = ctx.rmse_host(cells, regen, units, n)
        for i, b in enumerate(boxes):
            assert abs(rmse[i] - ref[i]) <= 1e-12 * abs(ref[i]), (i, rmse[i], ref[i])
            if b.size:
                o = units[i].cell_offset
                cpu = oracle.rmse(b, regen[o:o + b.size].reshape(b.shape))
                assert abs(rmse[i] - cpu) <= 1e-12 * abs(cpu), (i, rmse[i], cpu)
            print(f"unit {i} dims {DIMS[i]} tol {TOL_A[i]:g} bound {bound[i]:.6g} rmse {rmse[i]:.6g}")
            if TOL_A[i] >= 1e-3:
                assert rmse[i] <= TOL_A[i] * (1 + MARGIN), (i, DIMS[i], TOL_A[i], rmse[i])


def test_odd_dimension_is_rejected(wc, ctx, expect):
    """A unit with cells and an odd dimension anywhere in the batch:
    WC_ERR_INVALID naming the unit, nothing written, and the context goes on."""
    dims = [(16, 16, 16), (4, 3, 2), (2, 2, 2)]
    units, n, extent = wc.capi.make_units(dims)
    cells = np.ones(extent, np.float32)
    d = Dev(wc, cells, units, n)
    for call in (lambda: ctx.forward_tol(d.cells.data_ptr(), d.dtype, units, n, 0.1, *d.out_args()),
                 lambda: ctx.forward_tol_host(cells, units, n, [0.1, 0.1, 0.1])):
        with pytest.raises(wc.WaveletError) as ei:
            call()
        assert ei.value.code == wc.capi.WC_ERR_INVALID and "unit 1" in str(ei.value) and "even" in str(ei.value)
    ctx.forward_stage(d.cells.data_ptr(), d.dtype, units, n, None)
    with pytest.raises(wc.WaveletError) as ei:
        ctx.forward_emit_tol(units, n, 0.1, *d.out_args())
    assert ei.value.code == wc.capi.WC_ERR_INVALID
    for bad in (-1.0, math.nan):
        with pytest.raises(wc.WaveletError) as ei:
            ctx.forward_tol(d.cells.data_ptr(), d.dtype, units, n, [0.1, 0.1, bad], *d.out_args())
        assert ei.value.code == wc.capi.WC_ERR_INVALID
    ctx.synchronize()
    _, kept, _, thresh, _ = d.read()
    assert (kept.view(np.int32) == -1).all() and (thresh == -7.0).all()  # nothing was launched
    boxes, units, n, extent, cells = make_batch(wc, np.float32)
    check_outputs(forward_tol(wc, ctx, cells, units, n, TOL_B), boxes, units, TOL_B, expect)


def run_cli(*args):
    r = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, WCAMD_THREADS="4"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[error]" not in r.stderr, r.stderr
    return r.stdout


def test_cli_rmse_reference_fixture():
    """-c with `rmse=` then -d on the reference's fixture plotfiles (even boxes
    16x32x64 and 8x4x2, tests/ref_plotfiles.py): every regenerated box within the
    tolerance.  Their fields are constant, so this checks the plumbing; the
    varying fields are in test_cli_rmse_round_trip."""
    from ref_plotfiles import write_ref_plotfiles
    from wavelet_compression_amd import plotfile as pf
    base = digit_free_dir()
    try:
        write_ref_plotfiles(base / "data")
        tol = 0.1
        run_cli(f"datadir={base}/data/", "minfile=plt00074", "maxfile=plt00075", "minlevel=0", "maxlevel=1",
                "components=temp pressure", f"rmse={tol}", f"compresseddir={base}/comp/", "-c")
        run_cli(f"compresseddir={base}/comp/", f"out={base}/regen/", "-d")
        for name in ("plt00074", "plt00075"):
            for lev in (0, 1):
                orig, regen = pf.read_level(base / "data" / name, lev), pf.read_level(base / "regen" / name, lev)
                assert len(orig) == len(regen) == 2
                for a, b in zip(orig, regen):
                    assert a.lo == b.lo and a.data.shape == b.data.shape
                    for c in range(2):
                        d = a.data[c].astype(np.float32).astype(np.float64) - b.data[c]
                        assert math.sqrt(float(np.mean(d * d))) <= tol * (1 + MARGIN), (name, lev, a.lo, c)
    finally:
        shutil.rmtree(base, ignore_errors=True)


def test_cli_rmse_round_trip(oracle):
    """-c with `rmse=` (one tolerance per component) then -d: every regenerated
    box is within its component's tolerance of the original; -estimate reports
    the actual RMSE of the same payloads.  The plotfile is written here with the
    project's writer, with fields that vary (|x| <= 8)."""
    from wavelet_compression_amd import plotfile as pf
    base = digit_free_dir()
    try:
        names, tols = ["temp", "pressure"], [0.05, 1e-3]
        boxes = [((0, 0, 0), (16, 16, 24)), ((16, 0, 0), (32, 32, 8)), ((0, 16, 0), (4, 2, 6))]
        fabs = [(lo, np.stack([field(c * 2, *d, seed=7 + 3 * b + c) for c in range(2)]).astype(np.float64))
                for b, (lo, d) in enumerate(boxes)]
        pf.write_plotfile(base / "data" / "plt00010", names, 1.25, [0.0, -1.0, 0.5, 1.0, 1.0, 2.5], 2, (64, 64, 32),
                          [100], [fabs])
        common = (f"datadir={base}/data/", "minfile=plt00010", "maxfile=plt00010", "minlevel=0", "maxlevel=0",
                  "components=temp pressure", "rmse=0.05 1e-3", "keep=0.999")
        out = run_cli(*common, f"compresseddir={base}/comp/", "-c")
        assert "keep is ignored" in out
        run_cli(f"compresseddir={base}/comp/", f"out={base}/regen/", "-d")
        regen = pf.read_level(base / "regen" / "plt00010", 0)
        per_comp = [[], []]
        for (lo, orig), fab in zip(fabs, regen):
            assert tuple(fab.lo) == tuple(lo)
            for c in range(2):
                r = oracle.rmse(orig[c].astype(np.float32), fab.data[c].astype(np.float32))
                print(f"box {lo} comp {names[c]} tol {tols[c]:g} rmse {r:.6g}")
                assert r <= tols[c] * (1 + MARGIN), (lo, names[c], r)
                per_comp[c].append(r)
        assert per_comp[0][0] > 0.0  # the tolerance is binding somewhere: coefficients were dropped
        est = run_cli(*common, f"compresseddir={base}/unused/", "-estimate")
        got = {k: float(v) for k, v in re.findall(r"Predicted RMSE, (\w+) = (\S+)", est)}
        for c in range(2):
            mean = sum(per_comp[c]) / len(per_comp[c])
            assert got[names[c]] == pytest.approx(mean, rel=1e-12, abs=1e-300)
    finally:
        shutil.rmtree(base, ignore_errors=True)
