"""GPU: the reduced-resolution decode (include/wavelet_amd.h wc_inverse_coarse,
wc_inverse_coarse_host, codec.decompress(coarsen=), the C++ mirror's
decompress_coarse) against the CPU restatement coarse_ref.py.

Bar: bit for bit on cells.  Every element of the output buffer that no unit
owns must keep its sentinel.  The data here is finite; payloads of NaN, +-inf,
-0 and subnormal cells at random shapes and reductions are in
tests/test_gpu_modes_fuzz.py.

Shapes, the smallest that reach each path: 2^3 L1 r1 (a corner of one
coefficient), 4^3 L2, 8^3 L3, 16^3 L4 at every r (the last level is one 2x2x2
block; odd block counts along K), 12x20x8 L2 and 16x8x24 L3 at every r (unequal
axes), 32x32x8 L1 / L2 at r = 1 and 64^3 L3 from fp64 data (fast inverse tiles;
about 14 pair tiles at keep 0.999, the corner's end inside a tile, later tiles
leaving early), one 128^3 L4 unit at r = 1 and r = 4 (several workgroups per
pass).  Beside them: units with r = 0, units without cells, an odd output cell
offset, keep = 1.5 (every coefficient kept: pair index = position), a payload
without pairs (keep = 0) and one with surplus pairs past ncoeff."""
import lzma
import subprocess
from pathlib import Path

import numpy as np
import pytest

import coarse_ref as C
import levels_ref as R
from tol_rule import field
from wavelet_compression_amd.capi import (WC_OPT_HOST_CHUNK, WC_OPT_ORDERED, WC_OPT_REVERSE_TILES,
                                          WC_OPT_SPIN_LIMIT, WcUnit)

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TEST_BIN = ROOT / "tools" / "bin" / "test_coarse"
SENTINEL = -77.0
KEEPS = (0.0, 0.99, 0.999, 1.5)


def surplus(oracle, pay, extra=5):
    """The payload with `extra` pairs appended: they land past ncoeff and are dropped."""
    (W, H, D), nc, runs, vals = oracle.parse_payload(pay)
    runs = np.concatenate([runs, np.arange(extra, dtype=np.int32)])
    vals = np.concatenate([vals, np.full(extra, 9.0, np.float32)])
    return oracle.serialize(W, H, D, nc, runs, vals)


class Case:
    """One batch: payload bytes per unit, levels, reduces, the output layout and
    the reference cells (computed once, left unchanged)."""

    def __init__(self, wc, pays, reduce, odd_at=None):
        self.pays, self.reduce, self.n = list(pays), list(reduce), len(pays)
        self.dims, self.levels = [], []
        for p in self.pays:
            h = np.frombuffer(p[:20], "<i4")
            self.dims.append((int(h[0]), int(h[1]), int(h[2])))
            self.levels.append(C.payload_levels(p))
        self.units, _, _ = wc.capi.make_units(self.dims)
        self.cdims = [C.coarse_dims(*d, r) for d, r in zip(self.dims, self.reduce)]
        offs, cur = [], 0
        for i, (w, h, d) in enumerate(self.cdims):
            cur = (cur + 3) // 4 * 4
            if i == odd_at:
                cur += 1  # an odd output cell offset
            offs.append(cur)
            cur += w * h * d
        self.out_units, _, self.extent = wc.capi.make_units(self.cdims, offs)
        self.extent = max(self.extent, cur) + 8  # a sentinel margin behind the last unit
        if odd_at is None:  # the packing wc_coarse_units gives
            cu, ext = wc.capi.coarse_units(self.units, self.n, self.reduce)
            assert [(u.cell_offset, u.nx, u.ny, u.nz) for u in cu[:self.n]] == \
                [(u.cell_offset, u.nx, u.ny, u.nz) for u in self.out_units[:self.n]]
            assert ext == cur
        self.offsets = np.zeros(max(self.n, 1), np.uint64)
        pos = 4
        for i, p in enumerate(self.pays):
            self.offsets[i] = pos
            pos += (len(p) + 4 + 7) // 8 * 8
        self.buf = np.zeros(pos + 8, np.uint8)
        for i, p in enumerate(self.pays):
            o = int(self.offsets[i])
            self.buf[o:o + len(p)] = np.frombuffer(p, np.uint8)
        self.want = [C.decode(p, r) for p, r in zip(self.pays, self.reduce)]

    def owned(self):
        m = np.zeros(self.extent, bool)
        for i, (w, h, d) in enumerate(self.cdims):
            o = self.out_units[i].cell_offset
            m[o:o + w * h * d] = True
        return m

    def check(self, cells, what="", skip=()):
        assert cells.size == self.extent
        for i, (w, h, d) in enumerate(self.cdims):
            if i in skip:
                continue
            o = self.out_units[i].cell_offset
            got = cells[o:o + w * h * d].reshape(d, h, w)
            assert got.tobytes() == self.want[i].tobytes(), (what, i, self.dims[i], self.levels[i], self.reduce[i])
        assert np.all(cells[~self.owned()] == SENTINEL), what  # nothing written outside the units


class Dev:
    def __init__(self, case):
        import torch
        dev = torch.device("cuda", 0)
        self.pay = torch.from_numpy(case.buf).to(dev)
        self.off = torch.from_numpy(case.offsets.view(np.int64)).to(dev)
        self.out = torch.full((case.extent,), SENTINEL, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()  # the fills run on torch's stream, the context on its own

    def refill(self):
        import torch
        self.out.fill_(SENTINEL)
        torch.cuda.synchronize()


def run_device(ctx, case, dev=None, levels="given", reduce=None, out_units=None):
    dev = dev or Dev(case)
    ctx.inverse_coarse(dev.pay.data_ptr(), dev.off.data_ptr(), case.units, case.n,
                       case.levels if levels == "given" else levels, case.reduce if reduce is None else reduce,
                       case.out_units if out_units is None else out_units, dev.out.data_ptr())
    ctx.synchronize()
    return dev.out.cpu().numpy()


def run_host(ctx, case, levels=None):
    out = np.full(case.extent, SENTINEL, np.float32)
    got = ctx.inverse_coarse_host(case.buf, case.offsets[:case.n], case.units, case.n, case.reduce, case.out_units,
                                  case.extent, levels=levels, out=out)
    return got


SMALL = [((2, 2, 2), 1, (1, 0)), ((4, 4, 4), 2, (1, 2)), ((8, 8, 8), 3, (1, 2, 3)), ((16, 16, 16), 4, (1, 2, 3, 4, 0)),
         ((12, 20, 8), 2, (0, 1, 2)), ((16, 8, 24), 3, (0, 1, 2, 3)), ((5, 7, 3), 1, (0,)), ((6, 10, 14), 1, (0, 1)),
         ((0, 4, 4), 1, (1,)), ((0, 8, 8), 2, (2,)), ((8, 8, 8), 1, (1,))]


def small_case(wc, oracle, keep):
    pays, reduce = [], []
    for i, (dims, L, rs) in enumerate(SMALL):
        W, H, D = dims
        box = field(i % 3, W, H, D, seed=60 + i) if W * H * D else np.zeros((D, H, W), np.float32)
        p = R.payload(box, L, keep=keep)[0]
        if keep == 1.5 and W * H * D >= 512 and int(np.frombuffer(p[16:20], "<i4")[0]) == W * H * D:
            p = surplus(oracle, p)  # every coefficient kept: the appended pairs land past ncoeff
        for r in rs:
            pays.append(p)
            reduce.append(r)
    return Case(wc, pays, reduce, odd_at=3)


@pytest.fixture(scope="module")
def small(wc, oracle):
    return {k: small_case(wc, oracle, k) for k in KEEPS}


@pytest.fixture(scope="module")
def fast(wc, oracle):
    """Multi-tile units: 64^3 L3 (fp64 data narrowed) at every r and at keep 0.999
    and 1.5 (64 pair tiles, pair index = position), 32x32x8 at L = 1, 2."""
    def box(i, d):
        return oracle.narrow(oracle.synth_box_f64(oracle.unit_seed(0, 0, 3 + i, 1), (0, 0, 0), *d))
    b64, b32 = box(1, (64, 64, 64)), box(0, (32, 32, 8))
    p999, pall = R.payload(b64, 3, keep=0.999)[0], surplus(oracle, R.payload(b64, 3, keep=1.5)[0])
    npairs = int(np.frombuffer(p999[16:20], "<i4")[0])
    assert 8 * 4096 < npairs < 20 * 4096  # several pair tiles, far fewer than the 64 of the dense array
    assert int(np.frombuffer(pall[16:20], "<i4")[0]) == 64 ** 3 + 5  # everything kept, and the surplus pairs
    pays = [R.payload(b32, 1, keep=0.999)[0], R.payload(b32, 2, keep=0.999)[0], p999, p999, p999, p999, pall, pall,
            R.payload(box(2, (64, 64, 64)), 1, keep=0.999)[0]]
    return Case(wc, pays, [1, 1, 1, 2, 3, 0, 1, 3, 1])


@pytest.fixture(scope="module")
def big(wc, oracle):
    b = oracle.narrow(oracle.synth_box_f64(oracle.unit_seed(0, 0, 3, 1), (0, 0, 0), 128, 128, 128))
    p = R.payload(b, 4, keep=0.999)[0]
    return Case(wc, [p, p], [1, 4])


def test_small_shapes_every_reduce(wc, ctx, small):
    for keep, case in small.items():
        assert any(w * h * d == 1 for w, h, d in case.cdims)  # a corner of one coefficient
        case.check(run_device(ctx, case), what=("device", keep))
        for lv in (case.levels, None):  # given, or read from the headers
            case.check(run_host(ctx, case, lv), what=("host", keep, lv is None))
    # the batches hold what they claim: payloads of boxes with cells that have no pair
    # (keep 0 with a positive signed maximum), and payloads with every coefficient kept
    # (keep 1.5 with a positive signed maximum: pair index = position), one of them with surplus pairs
    def pairs(p):
        return int(np.frombuffer(p[16:20], "<i4")[0])
    assert any(pairs(p) == 0 and np.prod(d) > 0 for p, d in zip(small[0.0].pays, small[0.0].dims))
    assert any(pairs(p) == np.prod(d) > 1 for p, d in zip(small[1.5].pays, small[1.5].dims))
    assert any(pairs(p) > np.prod(d) > 1 for p, d in zip(small[1.5].pays, small[1.5].dims))


def test_fast_tiles_and_early_exits(wc, ctx, fast):
    fast.check(run_device(ctx, fast), what="device")
    fast.check(run_host(ctx, fast), what="host")


def test_one_large_unit(wc, ctx, big):
    big.check(run_device(ctx, big), what="device")


def test_lookback_forms_give_the_same_cells(wc, ctx, fast, small):
    """Ticket form, reversed launch order and a wait bound of one poll: the
    existing hooks, on the batch with multi-tile units."""
    for opt, val, back in ((WC_OPT_ORDERED, 0, 1), (WC_OPT_REVERSE_TILES, 1, 0), (WC_OPT_SPIN_LIMIT, 1, 0)):
        ctx.set_option(opt, val)
        try:
            fast.check(run_device(ctx, fast), what=(opt, val))
            small[0.999].check(run_device(ctx, small[0.999]), what=(opt, val, "small"))
        finally:
            ctx.set_option(opt, back)
    ctx.set_option(WC_OPT_REVERSE_TILES, 1)
    ctx.set_option(WC_OPT_SPIN_LIMIT, 1)
    try:
        fast.check(run_device(ctx, fast), what="reversed, one poll")
    finally:
        ctx.set_option(WC_OPT_REVERSE_TILES, 0)
        ctx.set_option(WC_OPT_SPIN_LIMIT, 0)


def test_odd_direct_partial_empty_and_multi_tile_units_in_one_batch(wc, ctx, fast):
    """One batch of the decode kernel's whole-box form under each look-back form:
    an odd unit at L = 1, r = 0 (the region map is not stated for it), a unit
    with r = L, one with 0 < r < L, one without cells, and a unit of the `fast`
    batch whose payload spans more than two pair tiles."""
    mix = [((5, 6, 7), 1, 0), ((16, 16, 16), 2, 2), ((16, 8, 24), 3, 2), ((0, 4, 4), 1, 1)]
    pays = [R.payload(field(i % 3, W, H, D, seed=80 + i) if W * H * D else np.zeros((D, H, W), np.float32), L,
                      keep=0.99)[0] for i, ((W, H, D), L, _) in enumerate(mix)]
    assert fast.dims[2] == (64, 64, 64) and int(np.frombuffer(fast.pays[2][16:20], "<i4")[0]) > 2 * 4096
    case = Case(wc, pays + [fast.pays[2]], [r for _, _, r in mix] + [1])
    assert case.levels == [1, 2, 3, 1, 3]
    dev = Dev(case)
    for what, opt, val, back in (("ordered", None, 0, 0), ("tickets", WC_OPT_ORDERED, 0, 1),
                                 ("reversed", WC_OPT_REVERSE_TILES, 1, 0)):
        if opt is not None:
            ctx.set_option(opt, val)
        try:
            dev.refill()
            case.check(run_device(ctx, case, dev), what=what)
        finally:
            if opt is not None:
                ctx.set_option(opt, back)


def test_host_form_in_several_runs(wc, ctx, fast, small):
    want = {id(c): run_device(ctx, c) for c in (fast, small[0.99])}
    ctx.set_option(WC_OPT_HOST_CHUNK, 3000)
    try:
        for c in (fast, small[0.99]):
            got = run_host(ctx, c)
            c.check(got, what="host runs")
            assert got.tobytes() == want[id(c)].tobytes()
    finally:
        ctx.set_option(WC_OPT_HOST_CHUNK, 1 << 25)


def test_all_zero_reduce_is_the_full_inverse(wc, ctx, oracle):
    import torch
    boxes = [field(0, 8, 8, 8, 1), field(2, 12, 20, 8, 2), field(1, 5, 7, 3, 3), field(0, 32, 32, 8, 4)]
    for levels in ([3, 2, 1, 2], [1, 1, 1, 1]):
        pays = [R.payload(b, L, keep=0.99)[0] for b, L in zip(boxes, levels)]
        case = Case(wc, pays, [0] * len(pays), odd_at=2)
        d = Dev(case)
        got = run_device(ctx, case, d, levels=None if levels == [1, 1, 1, 1] else "given")
        case.check(got, what=("all zero", levels))
        d2 = Dev(case)
        if levels == [1, 1, 1, 1]:
            ctx.inverse(d2.pay.data_ptr(), d2.off.data_ptr(), case.out_units, case.n, d2.out.data_ptr())
        else:
            ctx.inverse_levels(d2.pay.data_ptr(), d2.off.data_ptr(), case.out_units, case.n, levels, d2.out.data_ptr())
        ctx.synchronize()
        assert got.tobytes() == d2.out.cpu().numpy().tobytes()
        case.check(run_host(ctx, case), what=("all zero host", levels))
    torch.cuda.synchronize()


def test_invalid_arguments_are_refused_before_any_launch(wc, ctx):
    import ctypes
    INVALID = wc.capi.WC_ERR_INVALID
    boxes = [field(0, 8, 8, 8, 1), field(0, 6, 5, 8, 2), field(1, 4, 4, 4, 3)]
    levels = [2, 1, 2]
    case = Case(wc, [R.payload(b, L, keep=0.99)[0] for b, L in zip(boxes, levels)], [1, 0, 2])
    d = Dev(case)

    def units_with(i, **kw):
        u = (WcUnit * case.n)(*[WcUnit(x.cell_offset, x.nx, x.ny, x.nz, x.reserved) for x in case.out_units[:case.n]])
        for k, v in kw.items():
            setattr(u[i], k, v)
        return u

    halved = units_with(1, nx=3, ny=2, nz=4)
    bad = [
        (dict(reduce=[1, 0, -1]), "unit 2"),   # a reduce outside 0..L
        (dict(reduce=[1, 0, 3]), "unit 2"),
        (dict(reduce=[3, 0, 2]), "unit 0"),
        (dict(reduce=[1, 2, 2], out_units=halved), "unit 1"),
        (dict(reduce=[1, 1, 2], out_units=halved), "unit 1"),   # 6x5x8: 2 does not divide H
        (dict(out_units=units_with(0, nx=8)), "unit 0"),        # other dims
        (dict(out_units=units_with(2, nz=2)), "unit 2"),
        (dict(out_units=units_with(1, reserved=1)), "unit 1"),
        (dict(levels=[2, 1, 5]), "unit 2"),                     # the levels rule itself
        (dict(levels=[2, 2, 2]), "unit 1"),
    ]
    for kw, word in bad:
        with pytest.raises(wc.WaveletError) as ei:
            run_device(ctx, case, d, **kw)
        assert ei.value.code == INVALID and word in str(ei.value), (kw, str(ei.value))
        out = np.full(case.extent, SENTINEL, np.float32)
        with pytest.raises(wc.WaveletError) as ei:
            ctx.inverse_coarse_host(case.buf, case.offsets[:case.n], case.units, case.n, kw.get("reduce", case.reduce),
                                    kw.get("out_units", case.out_units), case.extent,
                                    levels=kw.get("levels", case.levels), out=out)
        assert ei.value.code == INVALID and word in str(ei.value), ("host", kw, str(ei.value))
        assert np.all(out == SENTINEL)
    # levels = NULL on the device form means all 1: reduce 2 of unit 2 is then beyond its levels
    with pytest.raises(wc.WaveletError) as ei:
        run_device(ctx, case, d, levels=None)
    assert ei.value.code == INVALID and "unit 2" in str(ei.value)
    # null buffers
    for args in ((0, d.off.data_ptr(), d.out.data_ptr()), (d.pay.data_ptr(), 0, d.out.data_ptr()),
                 (d.pay.data_ptr(), d.off.data_ptr(), 0)):
        with pytest.raises(wc.WaveletError) as ei:
            ctx.inverse_coarse(args[0], args[1], case.units, case.n, case.levels, case.reduce, case.out_units, args[2])
        assert ei.value.code == INVALID and "null" in str(ei.value)
    L = wc.capi.load_library()
    lv, rd = np.array(case.levels, np.int32), np.array(case.reduce, np.int32)
    pay, off, out = (ctypes.c_void_p(t.data_ptr()) for t in (d.pay, d.off, d.out))
    assert L.wc_inverse_coarse(ctx.handle, pay, off, case.units, case.n, lv.ctypes.data, None, case.out_units,
                               out) == INVALID
    assert L.wc_inverse_coarse(ctx.handle, pay, off, case.units, case.n, lv.ctypes.data, rd.ctypes.data, None,
                               out) == INVALID
    ctx.synchronize()
    assert bool((d.out == SENTINEL).all())  # nothing was launched
    # the context goes on
    case.check(run_device(ctx, case, d), what="after refusals")


def patched(pay, word, value):
    b = bytearray(pay)
    b[4 * word:4 * word + 4] = np.array([value], "<i4").tobytes()
    return bytes(b)


def test_malformed_payloads(wc, ctx):
    FORMAT = wc.capi.WC_ERR_FORMAT
    boxes = [field(0, 8, 8, 8, 1), field(2, 16, 16, 16, 2), field(0, 8, 8, 8, 3), field(1, 4, 4, 4, 4)]
    levels = [2, 3, 3, 2]
    pays = [R.payload(b, L, keep=0.99)[0] for b, L in zip(boxes, levels)]
    reduce = [1, 2, 3, 2]
    good = Case(wc, pays, reduce)
    good.check(run_device(ctx, good), what="good")
    # a header carrying another L, other dims, or a negative pair count: that unit
    # (a level-pass unit, then a unit with r == L) is refused alone
    for i, word, value in ((1, 3, -2), (1, 2, 8), (2, 3, -2), (2, 0, 16), (0, 3, 512), (1, 4, -1)):
        bad_pays = list(pays)
        bad_pays[i] = patched(pays[i], word, value)
        case = Case.__new__(Case)
        case.__dict__.update(good.__dict__)
        case.buf = good.buf.copy()
        o = int(good.offsets[i])
        case.buf[o:o + len(pays[i])] = np.frombuffer(bad_pays[i], np.uint8)
        d = Dev(case)
        ctx.inverse_coarse(d.pay.data_ptr(), d.off.data_ptr(), case.units, case.n, levels, reduce, case.out_units,
                           d.out.data_ptr())
        with pytest.raises(wc.WaveletError) as ei:
            ctx.synchronize()
        assert ei.value.code == FORMAT, (i, word, value)
        ctx.synchronize()  # the error word is cleared
        cells = d.out.cpu().numpy()
        w, h, dd = case.cdims[i]
        o = case.out_units[i].cell_offset
        assert np.all(cells[o:o + w * h * dd] == SENTINEL), (i, word, value)  # the refused unit stays untouched
        case.check(cells, what=("neighbours", i, word, value), skip=(i,))
    # a negative run: the error, and nothing outside that unit's output range
    for i in (1, 2):
        (W, H, D), nc, runs, vals = wc_oracle_parse(pays[i])
        runs = runs.copy()
        runs[len(runs) // 2] = -2
        from oracle import oracle as O
        case = Case.__new__(Case)
        case.__dict__.update(good.__dict__)
        case.buf = good.buf.copy()
        o = int(good.offsets[i])
        case.buf[o:o + len(pays[i])] = np.frombuffer(O.serialize(W, H, D, nc, runs, vals), np.uint8)
        d = Dev(case)
        ctx.inverse_coarse(d.pay.data_ptr(), d.off.data_ptr(), case.units, case.n, levels, reduce, case.out_units,
                           d.out.data_ptr())
        with pytest.raises(wc.WaveletError) as ei:
            ctx.synchronize()
        assert ei.value.code == FORMAT and "flags 0x2" in str(ei.value)  # the negative-run bit alone
        ctx.synchronize()
        case.check(d.out.cpu().numpy(), what=("negative run", i), skip=(i,))
    # the host form refuses a header that is no payload header, naming the unit
    case = Case.__new__(Case)
    case.__dict__.update(good.__dict__)
    case.buf = good.buf.copy()
    o = int(good.offsets[1])
    case.buf[o + 12:o + 16] = np.frombuffer(np.array([-7], "<i4").tobytes(), np.uint8)
    with pytest.raises(wc.WaveletError) as ei:
        run_host(ctx, case)
    assert ei.value.code == FORMAT and "unit 1" in str(ei.value)
    with pytest.raises(wc.WaveletError) as ei:
        run_host(ctx, good, levels=[2, 3, 3, 3])  # 4^3 admits no third level
    assert ei.value.code == wc.capi.WC_ERR_INVALID
    # the context goes on
    good.check(run_device(ctx, good), what="after malformed")


def wc_oracle_parse(pay):
    from oracle import oracle as O
    return O.parse_payload(pay)


def test_codec_files_and_cpp_mirror(wc, oracle, tmp_path):
    """codec.compress(levels=3) -> decompress(coarsen=r) through .xz files, a
    reference-format file (levels = 1) at coarsen=1, and the C++ mirror's
    decompress_coarse on the same files: the Python result's bytes."""
    from wavelet_compression_amd import codec
    boxes = [field(0, 16, 8, 24, 5), field(2, 32, 32, 8, 6)]
    for levels, tag, rs in ((3, "multi", (0, 1, 2, 3)), (1, "plain", (0, 1))):
        cdir = tmp_path / tag
        cdir.mkdir()
        codec.compress(boxes, [0, 1], 0.999, 0, 0, 7, cdir, levels=levels)
        for c, box in enumerate(boxes):
            f = cdir / f"compressed-wavelet-0-0-{c}-7.xz"
            raw = lzma.decompress(f.read_bytes())
            assert C.payload_levels(raw) == levels
            if levels == 1:
                assert raw == oracle.compress_payload(box, 0.999)[0]  # the reference's own file format
            for r in rs:
                got = codec.decompress(str(f), coarsen=r)
                want = C.decode(raw, r)
                assert got.shape == want.shape and got.tobytes() == want.tobytes(), (tag, c, r)
                out = tmp_path / f"{tag}-{c}-{r}.raw"
                p = subprocess.run([str(TEST_BIN), str(f), str(r), str(out)], capture_output=True, text=True,
                                   timeout=120)
                assert p.returncode == 0, p.stdout + p.stderr
                W, H, D = box.shape[2] >> r, box.shape[1] >> r, box.shape[0] >> r
                assert p.stdout.split() == [str(W), str(H), str(D)]
                assert out.read_bytes() == got.tobytes(), (tag, c, r)
        # a reduction the file does not admit: the mirror exits with a message, the codec raises
        f = cdir / "compressed-wavelet-0-0-0-7.xz"
        p = subprocess.run([str(TEST_BIN), str(f), str(levels + 1), str(tmp_path / "none.raw")], capture_output=True,
                           text=True, timeout=120)
        assert p.returncode != 0 and "[error]" in p.stderr
        if levels < 4:
            with pytest.raises(ValueError, match="payload 0"):
                codec.decompress(str(f), coarsen=levels + 1)
    # batched: payloads of different levels at one coarsen
    pays = [R.payload(boxes[0], 3, keep=0.99)[0], oracle.compress_payload(boxes[1], 0.99)[0]]
    got = codec.decompress_payloads(pays, coarsen=1)
    for g, p in zip(got, pays):
        assert g.tobytes() == C.decode(p, 1).tobytes()
