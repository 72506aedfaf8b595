"""GPU: the sub-box decode (include/wavelet_amd.h wc_inverse_region,
wc_inverse_region_host, codec.decompress(region=), the C++ mirror's
decompress_region) against the CPU restatement region_ref.py.

Bar: bit for bit on cells.  Every element of the output buffer that no unit
owns must keep its sentinel.

Shapes, the smallest that reach each path: 2^3 L1 with the whole box; 4^3 L2,
8^3 L3, 16^3 L4 at every r with a one-block region (a 2^L cube) at the origin
and at the far corner (end = W*H*D); 12x20x8 L2 and 16x8x24 L3 with unequal
regions; 32x32x8 L1 / L2; 64^3 L3 from fp64 data at keep 0.999 (about 14 pair
tiles) with 8-thick slabs normal to x, y and z at the first, a middle and the
last position, at r = 0, 1 and 3 (x-first: end inside an early tile, later
tiles leaving; z slabs: strided hits in every tile); one 128^3 L4 unit with a
16-thick slab at r = 0 and r = 4.  Beside them, in the same batches: whole-box
regions, zero-extent regions, units without cells, an odd output offset, keep =
1.5 (pair index = position), payloads without pairs (keep = 0) and payloads
with surplus pairs past ncoeff."""
import lzma
import subprocess
from pathlib import Path

import numpy as np
import pytest

import coarse_ref as C
import levels_ref as R
import region_ref as G
from tol_rule import field
from wavelet_compression_amd.capi import (WC_OPT_HOST_CHUNK, WC_OPT_ORDERED, WC_OPT_REVERSE_TILES,
                                          WC_OPT_SPIN_LIMIT, WcUnit)

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TEST_BIN = ROOT / "tools" / "bin" / "test_region"
SENTINEL = -77.0
KEEPS = (0.0, 0.99, 0.999, 1.5)


def surplus(oracle, pay, extra=5):
    """The payload with `extra` pairs appended: they land past ncoeff and are dropped."""
    (W, H, D), nc, runs, vals = oracle.parse_payload(pay)
    runs = np.concatenate([runs, np.arange(extra, dtype=np.int32)])
    vals = np.concatenate([vals, np.full(extra, 9.0, np.float32)])
    return oracle.serialize(W, H, D, nc, runs, vals)


class Case:
    """One batch: payload bytes per unit, levels, reduces, regions, the output
    layout and the reference cells (computed once, left unchanged).  A region
    None is the whole box."""

    def __init__(self, wc, pays, reduce, regions, odd_at=None):
        self.pays, self.reduce, self.n = list(pays), list(reduce), len(pays)
        self.dims, self.levels = [], []
        for p in self.pays:
            h = np.frombuffer(p[:20], "<i4")
            self.dims.append((int(h[0]), int(h[1]), int(h[2])))
            self.levels.append(C.payload_levels(p))
        self.regions = [(0, 0, 0) + d if g is None else tuple(g) for g, d in zip(regions, self.dims)]
        self.units, _, _ = wc.capi.make_units(self.dims)
        self.cdims = [G.out_dims(g, r) for g, r in zip(self.regions, self.reduce)]
        offs, cur = [], 0
        for i, (w, h, d) in enumerate(self.cdims):
            cur = (cur + 3) // 4 * 4
            if i == odd_at:
                cur += 1  # an odd output cell offset
            offs.append(cur)
            cur += w * h * d
        self.out_units, _, self.extent = wc.capi.make_units(self.cdims, offs)
        self.extent = max(self.extent, cur) + 8  # a sentinel margin behind the last unit
        if odd_at is None:  # the packing wc_region_units gives
            cu, ext = wc.capi.region_units(self.units, self.n, self.regions, self.reduce)
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
        full = {}  # the full decode of a payload at a reduction, shared by the units that crop it

        def want(p, r, g):
            x0, y0, z0 = (v >> r for v in g[:3])
            w, h, d = G.out_dims(g, r)
            if w * h * d == 0:
                return np.zeros((d, h, w), np.float32)
            if (id(p), r) not in full:
                full[(id(p), r)] = C.decode(p, r)
            return np.ascontiguousarray(full[(id(p), r)][z0:z0 + d, y0:y0 + h, x0:x0 + w])

        self.want = [want(p, r, g) for p, r, g in zip(self.pays, self.reduce, self.regions)]

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
            assert got.tobytes() == self.want[i].tobytes(), \
                (what, i, self.dims[i], self.levels[i], self.reduce[i], self.regions[i])
        assert np.all(cells[~self.owned()] == SENTINEL), what  # nothing written outside the units


class Dev:
    def __init__(self, case):
        import torch
        dev = torch.device("cuda", 0)
        self.pay = torch.from_numpy(case.buf).to(dev)
        self.off = torch.from_numpy(case.offsets.view(np.int64)).to(dev)
        self.out = torch.full((case.extent,), SENTINEL, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()  # the fills run on torch's stream, the context on its own


def run_device(ctx, case, dev=None, levels="given", reduce="given", regions=None, out_units=None):
    dev = dev or Dev(case)
    ctx.inverse_region(dev.pay.data_ptr(), dev.off.data_ptr(), case.units, case.n,
                       case.levels if levels == "given" else levels, case.reduce if reduce == "given" else reduce,
                       case.regions if regions is None else regions,
                       case.out_units if out_units is None else out_units, dev.out.data_ptr())
    ctx.synchronize()
    return dev.out.cpu().numpy()


def run_host(ctx, case, levels=None):
    out = np.full(case.extent, SENTINEL, np.float32)
    return ctx.inverse_region_host(case.buf, case.offsets[:case.n], case.units, case.n, case.reduce, case.regions,
                                   case.out_units, case.extent, levels=levels, out=out)


def block(dims, L, far):
    m = 1 << L
    return (tuple(n - m for n in dims) if far else (0, 0, 0)) + (m, m, m)


# (dims, L, [(r, region)]); None: the whole box.  In 4^3 L2, 8^3 L3 and 16^3 L4 the
# one block at the origin is also the one at the far corner (end = W*H*D); the
# two differ in 12x20x8 and 16x8x24.
SMALL = [((2, 2, 2), 1, [(0, None), (1, None)])]
for _dims, _L in (((4, 4, 4), 2), ((8, 8, 8), 3), ((16, 16, 16), 4)):
    SMALL.append((_dims, _L, [(r, block(_dims, _L, far)) for r in range(_L + 1) for far in (False, True)]))
SMALL += [
    ((12, 20, 8), 2, [(0, (4, 8, 0, 8, 4, 8)), (1, (8, 0, 4, 4, 12, 4)), (2, (0, 16, 4, 12, 4, 4)), (1, None)] +
     [(r, block((12, 20, 8), 2, far)) for r in range(3) for far in (False, True)]),
    ((16, 8, 24), 3, [(0, (8, 0, 8, 8, 8, 16)), (1, (0, 0, 16, 16, 8, 8)), (2, (8, 0, 0, 8, 8, 24)),
                      (3, (0, 0, 8, 16, 8, 8)), (3, None), (0, None)] +
     [(r, block((16, 8, 24), 3, far)) for r in range(4) for far in (False, True)]),
    ((6, 10, 14), 1, [(0, (2, 4, 6, 4, 2, 8)), (1, (4, 0, 12, 2, 10, 2)), (1, None)]),
    ((8, 8, 8), 1, [(0, (6, 6, 6, 2, 2, 2)), (1, (0, 2, 4, 8, 2, 2))]),
    ((0, 4, 4), 1, [(1, (0, 0, 0, 0, 0, 0))]), ((0, 8, 8), 2, [(2, (0, 0, 0, 0, 0, 0))]),   # units without cells
    ((8, 8, 8), 2, [(1, (4, 4, 4, 0, 4, 4)), (0, (8, 8, 8, 0, 0, 0)), (2, (0, 4, 0, 4, 4, 0))]),  # zero extents
]


def small_case(wc, oracle, keep):
    pays, reduce, regions = [], [], []
    for i, (dims, L, rs) in enumerate(SMALL):
        W, H, D = dims
        box = field(i % 3, W, H, D, seed=80 + i) if W * H * D else np.zeros((D, H, W), np.float32)
        p = R.payload(box, L, keep=keep)[0]
        if keep == 1.5 and W * H * D >= 512 and int(np.frombuffer(p[16:20], "<i4")[0]) == W * H * D:
            p = surplus(oracle, p)  # every coefficient kept: the appended pairs land past ncoeff
        for r, g in rs:
            pays.append(p)
            reduce.append(r)
            regions.append(g)
    return Case(wc, pays, reduce, regions, odd_at=3)


@pytest.fixture(scope="module")
def small(wc, oracle):
    return {k: small_case(wc, oracle, k) for k in KEEPS}


def slabs(n, t):
    """t-thick slabs of an n^3 box normal to x, y and z at the first, a middle and the last position."""
    out = []
    for axis in range(3):
        for pos in (0, (n // 2 // t) * t - t, n - t):
            o, e = [0, 0, 0], [n, n, n]
            o[axis], e[axis] = pos, t
            out.append(tuple(o) + tuple(e))
    return out


@pytest.fixture(scope="module")
def fast(wc, oracle):
    """Multi-tile units: 64^3 L3 (fp64 data narrowed) at keep 0.999 with nine slabs
    at r = 0, 1, 3, the same at keep 1.5 with surplus pairs (64 pair tiles, pair
    index = position) on three slabs, 32x32x8 at L = 1, 2."""
    def box(i, d):
        return oracle.narrow(oracle.synth_box_f64(oracle.unit_seed(0, 0, 3 + i, 1), (0, 0, 0), *d))
    b64, b32 = box(1, (64, 64, 64)), box(0, (32, 32, 8))
    p999, pall = R.payload(b64, 3, keep=0.999)[0], surplus(oracle, R.payload(b64, 3, keep=1.5)[0])
    npairs = int(np.frombuffer(p999[16:20], "<i4")[0])
    assert 8 * 4096 < npairs < 20 * 4096  # several pair tiles, far fewer than the 64 of the dense array
    assert int(np.frombuffer(pall[16:20], "<i4")[0]) == 64 ** 3 + 5  # everything kept, and the surplus pairs
    p32 = [R.payload(b32, L, keep=0.999)[0] for L in (1, 2)]
    pays, reduce, regions = [], [], []
    for r in (0, 1, 3):
        for g in slabs(64, 8):
            pays.append(p999)
            reduce.append(r)
            regions.append(g)
    sl = slabs(64, 8)
    for r, g in ((0, sl[0]), (1, sl[4]), (3, sl[8]), (0, (24, 8, 40, 8, 8, 8)), (2, None)):
        pays.append(pall)
        reduce.append(r)
        regions.append(g)
    for p, r, g in ((p32[0], 0, (8, 16, 0, 16, 2, 8)), (p32[0], 1, (30, 0, 6, 2, 32, 2)), (p32[0], 1, None),
                    (p32[1], 0, (0, 28, 4, 32, 4, 4)), (p32[1], 2, (16, 16, 0, 16, 16, 8)), (p32[1], 1, None),
                    (p999, 0, (24, 8, 40, 8, 8, 8)), (p999, 0, None), (p999, 3, None), (p999, 0, (8, 8, 8, 8, 0, 8))):
        pays.append(p)
        reduce.append(r)
        regions.append(g)
    return Case(wc, pays, reduce, regions)


@pytest.fixture(scope="module")
def big(wc, oracle):
    b = oracle.narrow(oracle.synth_box_f64(oracle.unit_seed(0, 0, 3, 1), (0, 0, 0), 128, 128, 128))
    p = R.payload(b, 4, keep=0.999)[0]
    return Case(wc, [p, p], [0, 4], [(0, 48, 0, 128, 16, 128), (0, 0, 112, 128, 128, 16)])


def test_small_shapes_every_reduce(wc, ctx, small):
    for keep, case in small.items():
        assert any(w * h * d == 1 for w, h, d in case.cdims)  # a region of one coefficient
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
    # a far-corner block's end is the whole array, the origin block's is not
    assert G.index_map((16, 8, 24), 3, 0, block((16, 8, 24), 3, True))[2] == 16 * 8 * 24
    assert G.index_map((16, 8, 24), 3, 0, block((16, 8, 24), 3, False))[2] < 16 * 8 * 24


def test_slabs_and_early_exits(wc, ctx, fast):
    # x-first: end inside an early tile; the z slabs end in the last one
    ends = [G.index_map((64, 64, 64), 3, 0, g)[2] for g in slabs(64, 8)]
    assert ends[0] < 64 ** 3 * 5 // 8 and ends[8] == 64 ** 3
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


def test_host_form_in_several_runs(wc, ctx, fast, small):
    want = {id(c): run_device(ctx, c) for c in (fast, small[0.99])}
    ctx.set_option(WC_OPT_HOST_CHUNK, 3000)
    try:
        for c in (fast, small[0.99]):
            got = run_host(ctx, c)  # levels read from the headers
            c.check(got, what="host runs")
            assert got.tobytes() == want[id(c)].tobytes()
    finally:
        ctx.set_option(WC_OPT_HOST_CHUNK, 1 << 25)


def test_whole_box_is_the_coarse_and_the_full_inverse(wc, ctx, oracle):
    """R = the whole box: wc_inverse_coarse's output of the same call sequence, and
    with r = 0 wc_inverse_levels' (wc_inverse's at L = 1)."""
    boxes = [field(0, 8, 8, 8, 1), field(2, 12, 20, 8, 2), field(1, 6, 10, 14, 3), field(0, 32, 32, 8, 4)]
    for levels, reduce in (([3, 2, 1, 2], [1, 2, 1, 0]), ([3, 2, 1, 2], [0, 0, 0, 0]), ([1, 1, 1, 1], [0, 0, 0, 0])):
        pays = [R.payload(b, L, keep=0.99)[0] for b, L in zip(boxes, levels)]
        case = Case(wc, pays, reduce, [None] * 4, odd_at=2)
        d = Dev(case)
        ones = levels == [1, 1, 1, 1]
        got = run_device(ctx, case, d, levels=None if ones else "given", reduce=None if not any(reduce) else "given")
        case.check(got, what=("whole", levels, reduce))
        d2 = Dev(case)
        if any(reduce):
            ctx.inverse_coarse(d2.pay.data_ptr(), d2.off.data_ptr(), case.units, case.n, levels, reduce,
                               case.out_units, d2.out.data_ptr())
        elif ones:
            ctx.inverse(d2.pay.data_ptr(), d2.off.data_ptr(), case.out_units, case.n, d2.out.data_ptr())
        else:
            ctx.inverse_levels(d2.pay.data_ptr(), d2.off.data_ptr(), case.out_units, case.n, levels, d2.out.data_ptr())
        ctx.synchronize()
        assert got.tobytes() == d2.out.cpu().numpy().tobytes()
        case.check(run_host(ctx, case), what=("whole host", levels, reduce))


def test_invalid_arguments_are_refused_before_any_launch(wc, ctx):
    import ctypes
    INVALID = wc.capi.WC_ERR_INVALID
    boxes = [field(0, 8, 8, 8, 1), field(0, 6, 4, 8, 2), field(1, 4, 4, 4, 3), field(1, 6, 5, 8, 2)]
    levels = [2, 1, 2, 1]
    pays = [R.payload(b, L, keep=0.99)[0] for b, L in zip(boxes, levels)]
    case = Case(wc, pays[:3], [1, 0, 2], [(4, 0, 4, 4, 8, 4), (2, 0, 6, 4, 4, 2), None])
    d = Dev(case)

    def units_with(i, **kw):
        u = (WcUnit * case.n)(*[WcUnit(x.cell_offset, x.nx, x.ny, x.nz, x.reserved) for x in case.out_units[:case.n]])
        for k, v in kw.items():
            setattr(u[i], k, v)
        return u

    def regions_with(i, g):
        return [g if k == i else x for k, x in enumerate(case.regions)]

    bad = [
        (dict(reduce=[1, 0, -1]), "unit 2"),   # a reduce outside 0..L
        (dict(reduce=[1, 0, 3]), "unit 2"),
        (dict(reduce=[3, 0, 2]), "unit 0"),
        (dict(reduce=[1, 2, 2]), "unit 1"),
        (dict(regions=regions_with(0, (2, 0, 4, 4, 8, 4))), "unit 0"),    # an origin 2^L does not divide
        (dict(regions=regions_with(0, (4, 0, 4, 2, 8, 4))), "unit 0"),    # an extent 2^L does not divide
        (dict(regions=regions_with(1, (2, 0, 6, 4, 4, 4))), "unit 1"),    # past the box along z
        (dict(regions=regions_with(1, (-2, 0, 6, 4, 4, 2))), "unit 1"),   # a negative origin
        (dict(regions=regions_with(2, (0, 0, 0, 4, -4, 4))), "unit 2"),   # a negative extent
        (dict(regions=regions_with(2, (0, 0, 0, 8, 4, 4))), "unit 2"),    # larger than the box
        (dict(out_units=units_with(0, nx=4)), "unit 0"),                  # other dims
        (dict(out_units=units_with(2, nz=2)), "unit 2"),
        (dict(out_units=units_with(1, reserved=1)), "unit 1"),
        (dict(levels=[2, 1, 5]), "unit 2"),                               # the levels rule itself
        (dict(levels=[2, 2, 2]), "unit 1"),
    ]
    for kw, word in bad:
        with pytest.raises(wc.WaveletError) as ei:
            run_device(ctx, case, d, **kw)
        assert ei.value.code == INVALID and word in str(ei.value), (kw, str(ei.value))
        out = np.full(case.extent, SENTINEL, np.float32)
        with pytest.raises(wc.WaveletError) as ei:
            ctx.inverse_region_host(case.buf, case.offsets[:case.n], case.units, case.n, kw.get("reduce", case.reduce),
                                    kw.get("regions", case.regions), kw.get("out_units", case.out_units), case.extent,
                                    levels=kw.get("levels", case.levels), out=out)
        assert ei.value.code == INVALID and word in str(ei.value), ("host", kw, str(ei.value))
        assert np.all(out == SENTINEL)
    # a dimension 2^L does not divide (6x5x8 at L = 1), and a unit without cells with a region that is not all zero
    for p, g, og in ((pays[3], (0, 0, 0, 2, 2, 2), (2, 2, 2)),
                     (R.payload(np.zeros((4, 4, 0), np.float32), 1, keep=0.99)[0], (0, 0, 0, 0, 2, 2), (0, 2, 2))):
        odd = Case(wc, [pays[0], p], [0, 0], [None, (0, 0, 0, 0, 0, 0)])
        ou, _, _ = wc.capi.make_units([odd.cdims[0], og], [0, 512])
        assert odd.extent >= 512 + 8
        with pytest.raises(wc.WaveletError) as ei:
            run_device(ctx, odd, Dev(odd), regions=[odd.regions[0], g], out_units=ou)
        assert ei.value.code == INVALID and "unit 1" in str(ei.value), str(ei.value)
    # levels = NULL on the device form means all 1: reduce 2 of unit 2 is then beyond its levels
    with pytest.raises(wc.WaveletError) as ei:
        run_device(ctx, case, d, levels=None)
    assert ei.value.code == INVALID and "unit" in str(ei.value)
    # null buffers
    for args in ((0, d.off.data_ptr(), d.out.data_ptr()), (d.pay.data_ptr(), 0, d.out.data_ptr()),
                 (d.pay.data_ptr(), d.off.data_ptr(), 0)):
        with pytest.raises(wc.WaveletError) as ei:
            ctx.inverse_region(args[0], args[1], case.units, case.n, case.levels, case.reduce, case.regions,
                               case.out_units, args[2])
        assert ei.value.code == INVALID and "null" in str(ei.value)
    L = wc.capi.load_library()
    lv, rd = np.array(case.levels, np.int32), np.array(case.reduce, np.int32)
    rg = wc.capi.make_regions(case.regions, case.n)
    pay, off, out = (ctypes.c_void_p(t.data_ptr()) for t in (d.pay, d.off, d.out))
    assert L.wc_inverse_region(ctx.handle, pay, off, case.units, case.n, lv.ctypes.data, rd.ctypes.data, None,
                               case.out_units, out) == INVALID
    assert L.wc_inverse_region(ctx.handle, pay, off, case.units, case.n, lv.ctypes.data, rd.ctypes.data, rg, None,
                               out) == INVALID
    ctx.synchronize()
    assert bool((d.out == SENTINEL).all())  # nothing was launched
    # the context goes on
    case.check(run_device(ctx, case, d), what="after refusals")


def patched(pay, word, value):
    b = bytearray(pay)
    b[4 * word:4 * word + 4] = np.array([value], "<i4").tobytes()
    return bytes(b)


def with_payload(good, i, new):
    case = Case.__new__(Case)
    case.__dict__.update(good.__dict__)
    case.buf = good.buf.copy()
    o = int(good.offsets[i])
    assert len(new) == len(good.pays[i])
    case.buf[o:o + len(new)] = np.frombuffer(new, np.uint8)
    return case


def test_malformed_payloads(wc, ctx, oracle):
    """A wrong header and a negative run: the error at wc_synchronize, the other
    units intact.  Neither can store outside its unit: every store of the region
    decode is bounded by the descriptor alone (wc_region.hip, Bounds)."""
    FORMAT = wc.capi.WC_ERR_FORMAT
    boxes = [field(0, 8, 8, 8, 1), field(2, 16, 16, 16, 2), field(0, 8, 8, 8, 3), field(1, 4, 4, 4, 4)]
    levels = [2, 3, 3, 2]
    pays = [R.payload(b, L, keep=0.99)[0] for b, L in zip(boxes, levels)]
    reduce = [1, 2, 3, 0]
    good = Case(wc, pays, reduce, [(4, 0, 4, 4, 8, 4), (8, 8, 0, 8, 8, 16), None, (0, 0, 0, 4, 4, 4)])
    good.check(run_device(ctx, good), what="good")
    # a header carrying another L, other dims, or a negative pair count: that unit
    # (a level-pass unit, then a unit with r == L) is refused alone
    for i, word, value in ((1, 3, -2), (1, 2, 8), (2, 3, -2), (2, 0, 16), (0, 3, 512), (1, 4, -1)):
        case = with_payload(good, i, patched(pays[i], word, value))
        d = Dev(case)
        ctx.inverse_region(d.pay.data_ptr(), d.off.data_ptr(), case.units, case.n, levels, reduce, case.regions,
                           case.out_units, d.out.data_ptr())
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
        (W, H, D), nc, runs, vals = oracle.parse_payload(pays[i])
        runs = runs.copy()
        runs[len(runs) // 2] = -2
        case = with_payload(good, i, oracle.serialize(W, H, D, nc, runs, vals))
        d = Dev(case)
        ctx.inverse_region(d.pay.data_ptr(), d.off.data_ptr(), case.units, case.n, levels, reduce, case.regions,
                           case.out_units, d.out.data_ptr())
        with pytest.raises(wc.WaveletError) as ei:
            ctx.synchronize()
        assert ei.value.code == FORMAT and "flags 0x2" in str(ei.value)  # the negative-run bit alone
        ctx.synchronize()
        case.check(d.out.cpu().numpy(), what=("negative run", i), skip=(i,))
    # the host form refuses a header that is no payload header, naming the unit
    case = with_payload(good, 1, patched(pays[1], 3, -7))
    with pytest.raises(wc.WaveletError) as ei:
        run_host(ctx, case)
    assert ei.value.code == FORMAT and "unit 1" in str(ei.value)
    with pytest.raises(wc.WaveletError) as ei:
        run_host(ctx, good, levels=[2, 3, 3, 3])  # 4^3 admits no third level
    assert ei.value.code == wc.capi.WC_ERR_INVALID
    # the context goes on
    good.check(run_device(ctx, good), what="after malformed")


def test_codec_files_and_cpp_mirror(wc, oracle, tmp_path):
    """codec.compress(levels=3) -> decompress(region=, coarsen=r) through .xz files
    with unaligned regions, a reference-format file (levels = 1), and the C++
    mirror's decompress_region on the same files: the Python result's bytes."""
    from wavelet_compression_amd import codec
    boxes = [field(0, 16, 8, 24, 5), field(2, 32, 32, 8, 6)]
    regs = [((3, 1, 2), (10, 8, 7)), ((0, 0, 0), (1, 1, 1)), ((15, 7, 7), (16, 8, 8))]  # inside both boxes
    for levels, tag, rs in ((3, "multi", (0, 1, 3)), (1, "plain", (0, 1))):
        cdir = tmp_path / tag
        cdir.mkdir()
        codec.compress(boxes, [0, 1], 0.999, 0, 0, 7, cdir, levels=levels)
        for c, box in enumerate(boxes):
            f = cdir / f"compressed-wavelet-0-0-{c}-7.xz"
            raw = lzma.decompress(f.read_bytes())
            assert C.payload_levels(raw) == levels
            for r in rs:
                full = C.decode(raw, r)
                for lo, hi in regs:
                    got = codec.decompress(str(f), coarsen=r, region=(lo, hi))
                    up = (1 << r) - 1
                    a, b = [v >> r for v in lo], [(v + up) >> r for v in hi]
                    want = np.ascontiguousarray(full[a[2]:b[2], a[1]:b[1], a[0]:b[0]])
                    assert got.shape == want.shape and got.tobytes() == want.tobytes(), (tag, c, r, lo, hi)
                    if (lo, hi) != regs[0]:
                        continue  # the mirror: one region per file and reduction
                    out = tmp_path / f"{tag}-{c}-{r}.raw"
                    p = subprocess.run([str(TEST_BIN), str(f), *map(str, lo + hi), str(r), str(out)],
                                       capture_output=True, text=True, timeout=120)
                    assert p.returncode == 0, p.stdout + p.stderr
                    assert p.stdout.split() == [str(v) for v in reversed(want.shape)]
                    assert out.read_bytes() == got.tobytes(), (tag, c, r, lo, hi)
        # what the file does not admit: the mirror exits with a message, the codec raises
        f = cdir / "compressed-wavelet-0-0-0-7.xz"
        for args in ((0, 0, 0, 17, 8, 8, 0), (4, 4, 4, 4, 8, 8, 0), (0, 0, 0, 4, 4, 4, levels + 1)):
            p = subprocess.run([str(TEST_BIN), str(f), *map(str, args), str(tmp_path / "none.raw")],
                               capture_output=True, text=True, timeout=120)
            assert p.returncode != 0 and "[error]" in p.stderr, args
        with pytest.raises(ValueError, match="not inside"):
            codec.decompress(str(f), region=((0, 0, 0), (17, 8, 8)))
    # batched: payloads of different levels, one region and one coarsen
    pays = [R.payload(boxes[0], 3, keep=0.99)[0], oracle.compress_payload(boxes[1], 0.99)[0]]
    got = codec.decompress_payloads(pays, coarsen=1, region=((5, 2, 1), (12, 7, 8)))
    for g, p in zip(got, pays):
        assert g.tobytes() == np.ascontiguousarray(C.decode(p, 1)[0:4, 1:4, 2:6]).tobytes()


def test_seeded_batch_with_specials(wc, ctx, oracle):
    """One seeded batch of the fuzz's generators (tests/modes_batches.py): random
    shapes, levels and keeps, NaN / +-inf units, and one unit of subnormal cells,
    each with a random aligned region and reduction."""
    import modes_batches as MB
    rng = np.random.default_rng(4242)
    B = MB.levels_batch(oracle, 3)
    pays, reduce, regions = [], [], []
    tiny = (rng.standard_normal((8, 8, 8)) * 1e-41).astype(np.float32)  # subnormal cells
    assert np.all(np.abs(tiny[tiny != 0]) < np.finfo(np.float32).tiny)
    items = [(MB.narrow(oracle, b, B.dtype), L) for b, L in zip(B.boxes, B.levels)] + [(tiny, 2), (tiny, 1)]
    special_units = {B.tags[t] for t in MB.SPECIAL_TAGS}
    for k, (b32, L) in enumerate(items):
        D, H, W = b32.shape
        if b32.size and (W | H | D) & ((1 << L) - 1):
            continue  # L = 1 with an odd dimension: no region decode
        keep = float(np.float32(rng.choice([rng.uniform(0.5, 0.99999), *MB.KEEPS])))
        pays.append(R.payload(b32, L, keep=keep)[0])
        m = 1 << L
        if not b32.size:
            reduce.append(int(rng.integers(0, L + 1)))
            regions.append((0, 0, 0, 0, 0, 0))
            continue
        g0 = [int(rng.integers(0, n // m)) * m for n in (W, H, D)]
        ge = [int(rng.integers(1, (n - o) // m + 1)) * m for n, o in zip((W, H, D), g0)]
        reduce.append(int(rng.integers(0, L + 1)))
        regions.append(None if k in special_units else tuple(g0 + ge))  # the specials' cells: the whole box
    case = Case(wc, pays, reduce, regions, odd_at=5)
    specials = [i for i, w in enumerate(case.want) if w.size and not np.isfinite(w).all()]
    assert len(pays) >= 15 and specials  # NaN or inf cells reach some region's output
    case.check(run_device(ctx, case), what="specials device")
    case.check(run_host(ctx, case), what="specials host")
