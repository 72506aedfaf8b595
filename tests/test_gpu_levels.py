"""GPU: the opt-in multi-level transform (include/wavelet_amd.h wc_forward_levels,
wc_decompose_levels, wc_inverse_levels, wc_inverse_flat_levels, their _host
forms, the CLI's `levels=`) against the CPU restatement levels_ref.py, which
composes the oracle's one-level routines on numpy sub-boxes.

Bar: bit for bit.  Flat coefficient arrays, payload bytes, kept counts and
slot offsets for the keep rule and for an explicit threshold, reconstructed
cells; the host variants equal the device calls; all-ones levels equal
wc_forward / wc_inverse; bad arguments and mismatching headers are refused
with their codes and touch nothing they promise not to.  The data here is
finite; NaN, +-inf, -0 and subnormal cells, random shapes and the look-back
option sets are in tests/test_gpu_modes_fuzz.py.

Shapes, the smallest that reach each path: 4^3 L2, 8^3 L3, 16^3 L4 (the last
level is one 2x2x2 block; odd block counts along K take the scalar pass),
12x20x8 L2 and 16x8x24 L3 (unequal axes, H/8 = 1), 32x32x8 L2 and 64^3 L3 in
fp64 (fast transform tiles, 64 flat tiles), 128^3 fp32 L4 (the 8-wave emit,
several workgroups per level pass and in the key pass); beside them L = 1
units: odd dims, 6x10x14, no cells, an odd cell offset."""
import lzma
import os
import shutil
import subprocess

import numpy as np
import pytest

import levels_ref as R
from test_cli import CLI, digit_free_dir
from tol_rule import field
from wavelet_compression_amd.capi import WC_OPT_HOST_CHUNK

pytestmark = pytest.mark.gpu

KEEPS = (0.0, 0.99, 0.999, 1.5)
THRESH = 0.05


def checker(W, H, D, A, seed):
    """A small smooth field plus a +-A checkerboard of period 2 on every axis:
    the largest |c| is a level-1 detail of the far corner octant (about A),
    outside the low-pass octant (about 0.1)."""
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    f = 0.1 * np.sin(0.3 * x + seed) * np.cos(0.2 * y) + A * (1 - 2 * ((x + y + z) & 1))
    return f.astype(np.float32)


def batch_small():
    """(dims, levels, boxes, offsets) of the fp32 batch: every small shape, the
    L = 1 units and the key cases in one call."""
    spec = [((4, 4, 4), 2, 0), ((8, 8, 8), 3, 1), ((16, 16, 16), 4, 0), ((12, 20, 8), 2, 2), ((16, 8, 24), 3, 0),
            ((5, 7, 3), 1, 1), ((6, 10, 14), 1, 0), ((0, 4, 4), 1, 0), ((2, 2, 2), 1, 1),
            ((8, 8, 8), 2, "const"), ((8, 8, 8), 2, "neg"), ((8, 8, 8), 2, "checker"), ((0, 8, 8), 2, 0)]
    dims, levels, boxes, offsets = [], [], [], []
    cur = 0
    for i, (d, L, kind) in enumerate(spec):
        W, H, D = d
        if W * H * D == 0:
            b = np.zeros((D, H, W), np.float32)
        elif kind == "const":
            b = np.full((D, H, W), 3.0, np.float32)
        elif kind == "neg":
            b = -np.abs(field(1, W, H, D, seed=40 + i)) - 1.0
        elif kind == "checker":
            b = checker(W, H, D, 7.0, i)
        else:
            b = field(kind, W, H, D, seed=40 + i)
        cur = (cur + 3) // 4 * 4
        if d == (2, 2, 2):
            cur += 1  # an odd cell offset
        dims.append(d)
        levels.append(L)
        boxes.append(b)
        offsets.append(cur)
        cur += b.size
    return dims, levels, boxes, offsets


def batch_fast(oracle):
    dims = [(32, 32, 8), (64, 64, 64), (4, 4, 4), (32, 32, 8)]
    levels = [2, 3, 2, 1]
    boxes = [oracle.synth_box_f64(oracle.unit_seed(0, 0, 3 + i, 1), (0, 0, 0), *d) for i, d in enumerate(dims)]
    return dims, levels, boxes, None


def batch_big(oracle):
    d = (128, 128, 128)
    return [d], [4], [oracle.narrow(oracle.synth_box_f64(oracle.unit_seed(0, 0, 3, 1), (0, 0, 0), *d))], None


class Batch:
    """One batch with its reference results, computed once and left unchanged."""

    def __init__(self, wc, oracle, spec, dtype):
        self.dims, self.levels, boxes, offsets = spec
        self.dtype = dtype
        self.units, self.n, self.extent = wc.capi.make_units(self.dims, offsets)
        self.cells = np.zeros(max(self.extent, 1), dtype)
        self.boxes = []  # as the codec sees them: narrowed to fp32
        for i, b in enumerate(boxes):
            o = self.units[i].cell_offset
            self.cells[o:o + b.size] = b.ravel().astype(dtype)
            self.boxes.append(oracle.narrow(b) if b.dtype == np.float64 else b)
        self._flat, self._pay, self._regen = {}, {}, {}

    def flat(self, i):
        if i not in self._flat:
            b = self.boxes[i]
            self._flat[i] = R.decompose(b, self.levels[i]) if b.size else np.zeros(0, np.float32)
        return self._flat[i]

    def payload(self, i, keep=None, thresh=None):
        key = (i, keep, thresh)
        if key not in self._pay:
            self._pay[key] = R.payload(self.boxes[i], self.levels[i], keep=keep, thresh=thresh)
        return self._pay[key]

    def regen(self, i, keep=None, thresh=None):
        key = (i, keep, thresh)
        if key not in self._regen:
            self._regen[key] = R.decode(self.payload(i, keep, thresh)[0])[0]
        return self._regen[key]


@pytest.fixture(scope="module")
def small(wc, oracle):
    return Batch(wc, oracle, batch_small(), np.float32)


@pytest.fixture(scope="module")
def fast(wc, oracle):
    return Batch(wc, oracle, batch_fast(oracle), np.float64)


@pytest.fixture(scope="module")
def big(wc, oracle):
    return Batch(wc, oracle, batch_big(oracle), np.float32)


class Dev:
    """Device buffers of one batch, prefilled with sentinels."""

    def __init__(self, wc, B):
        import torch
        dev = torch.device("cuda", 0)
        self.wc, self.B = wc, B
        self.code = wc.capi.WC_F64 if B.dtype == np.float64 else wc.capi.WC_F32
        self.cells = torch.from_numpy(B.cells).to(dev)
        self.cap = wc.capi.payload_bound(B.units, B.n)
        self.pay = torch.full((self.cap,), 0xA5, dtype=torch.uint8, device=dev)
        self.off = torch.full((B.n + 1,), -3, dtype=torch.int64, device=dev)
        self.kept = torch.full((B.n,), -1, dtype=torch.int32, device=dev)
        self.flat = torch.full((max(B.extent, 1),), -77.0, dtype=torch.float32, device=dev)
        self.out = torch.full((max(B.extent, 1),), -77.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()  # the fills run on torch's stream, the context on its own

    def out_args(self):
        return self.pay.data_ptr(), self.cap, self.off.data_ptr(), self.kept.data_ptr()

    def read(self):
        pay = self.pay.cpu().numpy()
        off = self.off.cpu().numpy().view(np.uint64)
        kept = self.kept.cpu().numpy().view(np.uint32)
        return [self.wc.capi.unit_payload(pay, off, kept, i) for i in range(self.B.n)], kept.copy(), off.copy()

    def untouched(self):
        return (bool((self.pay == 0xA5).all()) and bool((self.off == -3).all()) and bool((self.kept == -1).all())
                and bool((self.flat == -77.0).all()) and bool((self.out == -77.0).all()))


def check_forward(B, got, keep=None, thresh=None):
    payloads, kept, off = got
    slot = 4
    for i in range(B.n):
        want, k = B.payload(i, keep, thresh)
        what = (i, B.dims[i], B.levels[i], keep, thresh)
        assert int(kept[i]) == k, what
        assert payloads[i] == want, what
        assert int(off[i]) == slot, what  # the slot rule of wc_forward: unchanged
        slot += 24 + 8 * B.boxes[i].size
    assert int(off[B.n]) == int(off[B.n - 1]) + 20 + 8 * int(kept[B.n - 1])


def check_cells(B, cells, keep=None, thresh=None, what=""):
    for i in range(B.n):
        o, b = B.units[i].cell_offset, B.boxes[i]
        got = cells[o:o + b.size].reshape(b.shape)
        assert got.tobytes() == B.regen(i, keep, thresh).tobytes(), (what, i, B.dims[i], B.levels[i], keep, thresh)


def run_all(wc, ctx, B, keeps, host_chunk=None):
    d = Dev(wc, B)
    # the transform alone
    ctx.decompose_levels(d.cells.data_ptr(), d.code, B.units, B.n, B.levels, d.flat.data_ptr())
    ctx.synchronize()
    flat = d.flat.cpu().numpy()
    for i in range(B.n):
        o = B.units[i].cell_offset
        assert flat[o:o + B.boxes[i].size].tobytes() == B.flat(i).tobytes(), ("decompose", i, B.dims[i], B.levels[i])
    # ... and back: the reference's flat arrays through the synthesis alone
    ref_flat = np.full(max(B.extent, 1), -5.0, np.float32)
    for i in range(B.n):
        o = B.units[i].cell_offset
        ref_flat[o:o + B.boxes[i].size] = B.flat(i)
    import torch
    d.flat.copy_(torch.from_numpy(ref_flat))
    torch.cuda.synchronize()
    ctx.inverse_flat_levels(d.flat.data_ptr(), B.units, B.n, B.levels, d.out.data_ptr())
    ctx.synchronize()
    check_cells(B, d.out.cpu().numpy(), thresh=-1.0, what="inverse_flat")
    # forward + inverse for every keep and for an explicit threshold
    for keep, thresh in [(k, None) for k in keeps] + [(None, THRESH)]:
        ctx.forward_levels(d.cells.data_ptr(), d.code, B.units, B.n, B.levels, keep if keep is not None else 0.5,
                           thresh, *d.out_args())
        ctx.synchronize()
        got = d.read()
        check_forward(B, got, keep, thresh)
        ctx.inverse_levels(d.pay.data_ptr(), d.off.data_ptr(), B.units, B.n, B.levels, d.out.data_ptr())
        ctx.synchronize()
        check_cells(B, d.out.cpu().numpy(), keep, thresh, what="inverse")
        # host variants: the same payloads, packed; the same cells, levels given or read from the headers
        payload, offs, kept = ctx.forward_levels_host(B.cells, B.units, B.n, B.levels, keep if keep is not None else 0.5,
                                                      thresh)
        pos = 4
        for i in range(B.n):
            assert int(offs[i]) == pos and int(kept[i]) == int(got[1][i]), i
            assert wc.capi.unit_payload(payload, offs, kept, i) == got[0][i], i
            pos += 24 + 8 * int(kept[i])
        for lv in (B.levels, None):
            check_cells(B, ctx.inverse_levels_host(payload, offs[:B.n], B.units, B.n, B.extent, levels=lv), keep,
                        thresh, what="inverse host")
    return d


def test_small_shapes_and_key_cases(wc, ctx, small):
    B = small
    # the key cases are what they claim: a tie at index 0, a negative signed
    # max, and a largest |c| that is a level-1 detail outside the octant
    for i, (d, L) in enumerate(zip(B.dims, B.levels)):
        if d == (8, 8, 8) and L == 2:
            f = B.flat(i)
            j = int(np.argmax(np.abs(f)))
            if np.all(B.boxes[i] == 3.0):
                assert j == 0 and np.count_nonzero(f) == 8 and np.all(f[f != 0] == 3.0)  # eight equal maxima
            elif B.boxes[i].max() < 0:
                assert f[j] < 0
            else:
                W, H, D = d
                I, J, K = j // (H * D), (j // D) % H, j % D
                assert I >= W // 2 and J >= H // 2 and K >= D // 2 and abs(f[j]) > 6.0
    run_all(wc, ctx, B, KEEPS)
    # several unit runs on the host path
    ctx.set_option(WC_OPT_HOST_CHUNK, 3000)
    try:
        payload, offs, kept = ctx.forward_levels_host(B.cells, B.units, B.n, B.levels, 0.99)
        for i in range(B.n):
            assert wc.capi.unit_payload(payload, offs, kept, i) == B.payload(i, 0.99)[0], i
        check_cells(B, ctx.inverse_levels_host(payload, offs[:B.n], B.units, B.n, B.extent), 0.99, what="host runs")
    finally:
        ctx.set_option(WC_OPT_HOST_CHUNK, 1 << 25)


def test_fast_tiles_fp64(wc, ctx, fast):
    run_all(wc, ctx, fast, KEEPS)


def test_one_large_unit(wc, ctx, big):
    run_all(wc, ctx, big, KEEPS)


def test_all_ones_levels_equal_the_one_level_calls(wc, ctx, small, fast):
    for B in (small, fast):
        d = Dev(wc, B)
        ones = [1] * B.n
        ctx.forward(d.cells.data_ptr(), d.code, B.units, B.n, 0.999, *d.out_args())
        ctx.synchronize()
        want = d.read()
        ctx.inverse(d.pay.data_ptr(), d.off.data_ptr(), B.units, B.n, d.out.data_ptr())
        ctx.synchronize()
        want_cells = d.out.cpu().numpy().copy()
        e = Dev(wc, B)
        ctx.forward_levels(e.cells.data_ptr(), e.code, B.units, B.n, ones, 0.999, None, *e.out_args())
        ctx.synchronize()
        got = e.read()
        assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
        ctx.inverse_levels(e.pay.data_ptr(), e.off.data_ptr(), B.units, B.n, ones, e.out.data_ptr())
        ctx.synchronize()
        assert e.out.cpu().numpy().tobytes() == want_cells.tobytes()
        # an explicit threshold with one level: stage + emit
        ctx.forward_stage(d.cells.data_ptr(), d.code, B.units, B.n, None)
        ctx.forward_emit(B.units, B.n, 0.5, THRESH, *d.out_args())
        ctx.synchronize()
        want = d.read()
        ctx.forward_levels(e.cells.data_ptr(), e.code, B.units, B.n, ones, 0.5, THRESH, *e.out_args())
        ctx.synchronize()
        got = e.read()
        assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes()


def test_refusals(wc, ctx, small):
    INVALID, FORMAT = wc.capi.WC_ERR_INVALID, wc.capi.WC_ERR_FORMAT
    dims = [(8, 8, 8), (6, 8, 8), (4, 4, 4)]
    units, n, extent = wc.capi.make_units(dims)
    B = Batch.__new__(Batch)
    B.dims, B.units, B.n, B.extent, B.dtype = dims, units, n, extent, np.float32
    B.cells = np.arange(extent, dtype=np.float32) % 17 - 8
    d = Dev(wc, B)
    calls = []
    for lv, word in (([2, 1, 0], "unit 2"), ([2, 1, 5], "unit 2"), ([2, 2, 2], "unit 1")):
        calls += [
            (lambda lv=lv: ctx.forward_levels(d.cells.data_ptr(), d.code, units, n, lv, 0.99, None, *d.out_args()), word),
            (lambda lv=lv: ctx.decompose_levels(d.cells.data_ptr(), d.code, units, n, lv, d.flat.data_ptr()), word),
            (lambda lv=lv: ctx.inverse_flat_levels(d.cells.data_ptr(), units, n, lv, d.out.data_ptr()), word),
            (lambda lv=lv: ctx.inverse_levels(d.pay.data_ptr(), d.off.data_ptr(), units, n, lv, d.out.data_ptr()), word),
            (lambda lv=lv: ctx.forward_levels_host(B.cells, units, n, lv, 0.99), word),
        ]
    for call, word in calls:
        with pytest.raises(wc.WaveletError) as ei:
            call()
        assert ei.value.code == INVALID and word in str(ei.value), str(ei.value)
    ctx.synchronize()
    assert d.untouched()  # nothing was launched

    # a good L2 payload batch; wc_forward_levels leaves nothing staged
    lv = [2, 1, 2]
    ctx.forward_levels(d.cells.data_ptr(), d.code, units, n, lv, 0.99, None, *d.out_args())
    ctx.synchronize()
    kept_before = d.kept.cpu().numpy().copy()
    for emit in (lambda: ctx.forward_emit(units, n, 0.99, None, *d.out_args()),
                 lambda: ctx.forward_emit_tol(units, n, 0.1, *d.out_args())):
        with pytest.raises(wc.WaveletError) as ei:
            emit()
        assert ei.value.code == INVALID
    assert d.kept.cpu().numpy().tobytes() == kept_before.tobytes()
    pay, _, _ = d.read()
    assert [wc.capi.payload_levels(p) for p in pay] == lv

    # every one-level decoder refuses the L2 payloads instead of decoding garbage
    ctx.inverse(d.pay.data_ptr(), d.off.data_ptr(), units, n, d.out.data_ptr())
    with pytest.raises(wc.WaveletError) as ei:
        ctx.synchronize()
    assert ei.value.code == FORMAT
    ctx.synchronize()  # the error word is cleared
    # the wrong L: refused, that unit untouched; the units whose headers agree decode as usual
    import torch
    good = d.out.clone()
    torch.cuda.synchronize()
    ctx.inverse_levels(d.pay.data_ptr(), d.off.data_ptr(), units, n, lv, good.data_ptr())
    ctx.synchronize()
    for wrong in ([3, 1, 2], [1, 1, 2], [2, 1, 1]):
        out = good.clone().fill_(-77.0)
        torch.cuda.synchronize()
        ctx.inverse_levels(d.pay.data_ptr(), d.off.data_ptr(), units, n, wrong, out.data_ptr())
        with pytest.raises(wc.WaveletError) as ei:
            ctx.synchronize()
        assert ei.value.code == FORMAT, wrong
        for i in range(n):
            o, cnt = units[i].cell_offset, dims[i][0] * dims[i][1] * dims[i][2]
            if wrong[i] == lv[i]:
                assert bool((out[o:o + cnt] == good[o:o + cnt]).all()), (wrong, i)
            else:
                assert bool((out[o:o + cnt] == -77.0).all()), (wrong, i)  # the refused unit stays untouched
    # the host form reads the levels from the headers, and refuses a header that is none
    p, offs, kept = ctx.forward_levels_host(B.cells, units, n, lv, 0.99)
    bad = p.copy()
    bad[int(offs[0]) + 12:int(offs[0]) + 16] = np.frombuffer(np.array([-7], "<i4").tobytes(), np.uint8)
    with pytest.raises(wc.WaveletError) as ei:
        ctx.inverse_levels_host(bad, offs[:n], units, n, extent)
    assert ei.value.code == FORMAT and "unit 0" in str(ei.value)
    with pytest.raises(wc.WaveletError) as ei:
        ctx.inverse_levels_host(p, offs[:n], units, n, extent, levels=[1, 1, 2])
    assert ei.value.code == FORMAT
    # the context goes on
    run_all(wc, ctx, small, (0.99,))


def run_cli(*args):
    r = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, WCAMD_THREADS="4"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[error]" not in r.stderr, r.stderr
    return r.stdout


def test_cli_levels_round_trip(wc, oracle):
    """-c with `levels=3` then -d on a small plotfile with varying fields: every
    box file holds the restatement's payload at the levels wc_levels_for gives
    its box (8x8x8 -> 3, 16x16x24 -> 3, 32x32x8 -> 3, 12x20x8 -> 2, 4x2x6 -> 1),
    the regenerated cells equal the restatement's, -estimate reports their RMSE,
    and an archive written without levels= is the reference's and decodes as before."""
    from wavelet_compression_amd import plotfile as pf
    base = digit_free_dir()
    try:
        names, keep = ["temp", "pressure"], 0.99
        boxes = [((0, 0, 0), (16, 16, 24)), ((16, 0, 0), (32, 32, 8)), ((0, 16, 0), (4, 2, 6)), ((0, 32, 0), (12, 20, 8)),
                 ((16, 32, 0), (8, 8, 8))]
        fabs = [(lo, np.stack([field(c * 2, *d, seed=7 + 3 * b + c) for c in range(2)]).astype(np.float64))
                for b, (lo, d) in enumerate(boxes)]
        pf.write_plotfile(base / "data" / "plt00010", names, 1.25, [0.0, -1.0, 0.5, 1.0, 1.0, 2.5], 2, (64, 64, 32),
                          [100], [fabs])
        common = (f"datadir={base}/data/", "minfile=plt00010", "maxfile=plt00010", "minlevel=0", "maxlevel=0",
                  "components=temp pressure", f"keep={keep}")
        keepf = float(np.float32(keep))  # the reference's keep is a float
        for tag, want_levels in (("multi", 3), ("plain", 1)):
            extra = ("levels=3",) if want_levels > 1 else ()
            out = run_cli(*common, *extra, f"compresseddir={base}/{tag}/", "-c")
            assert ("levels=3 given" in out) == (want_levels > 1)
            run_cli(f"compresseddir={base}/{tag}/", f"out={base}/regen_{tag}/", "-d")
            regen = pf.read_level(base / f"regen_{tag}" / "plt00010", 0)
            rmses = [[], []]
            for b, ((lo, orig), fab) in enumerate(zip(fabs, regen)):
                assert tuple(fab.lo) == tuple(lo)
                for c in range(2):
                    box = orig[c].astype(np.float32)
                    L = wc.capi.levels_for(*boxes[b][1], want_levels)
                    assert L == R.levels_for(*boxes[b][1], want_levels)
                    raw = lzma.decompress((base / tag / f"compressed-wavelet-0-0-{c}-{b}.xz").read_bytes())
                    assert wc.capi.payload_levels(raw[:20]) == L, (tag, b, c)
                    want, _ = R.payload(box, L, keep=keepf)
                    assert raw == want, (tag, b, c)
                    if L == 1:
                        assert raw == oracle.compress_payload(box, keepf)[0]
                    cells = R.decode(want)[0]
                    assert fab.data[c].astype(np.float32).tobytes() == cells.tobytes(), (tag, b, c)
                    rmses[c].append(oracle.rmse(box, cells))
            if want_levels > 1:
                import re
                est = run_cli(*common, *extra, f"compresseddir={base}/unused/", "-estimate")
                got = {k: float(v) for k, v in re.findall(r"Predicted RMSE, (\w+) = (\S+)", est)}
                for c in range(2):
                    assert got[names[c]] == pytest.approx(sum(rmses[c]) / len(rmses[c]), rel=1e-9, abs=1e-300)
    finally:
        shutil.rmtree(base, ignore_errors=True)
