"""GPU: the RMSE tolerance on the multi-level transform (include/wavelet_amd.h
wc_forward_levels_tol / wc_forward_levels_tol_host, codec.compress_payloads(
levels=, rmse=)) against the numpy restatement of the per-level rule
(leveltol_rule.py) on levels_ref's final arrays.

Bar: per unit, the device's per-level thresholds and model bound equal the
rule's bit for bit (entries past the unit's L are 0.0f); the payload bytes equal
the oracle's RLE + serialize of the masked final array; kept counts and slot
offsets follow; the reconstruction through wc_inverse_levels equals
levels_ref.decode of those bytes (test_gpu_fuzz.same_cells: a NaN matches any
NaN); the solo and split binning paths and every look-back form give the same
outputs; the actual RMSE of the host form's round trip is within tol * (1 +
MARGIN) on the finite units with tol >= 1e-3 (test_leveltol_cpu.py derives the
margin for up to four levels).

One mixed batch, in fp32 and in fp64 (unit: purpose):
  4^3 L2 (level 2 is one block), 8^3 L3, 16^3 L4, 12x20x8 L2,
  48x16x80 L4 (rows straddle flat tiles; D >> 3 = 10 puts a level boundary
  inside a 16-B load), 64^3 L3 (64 flat tiles, the solo limit), 64x64x72 L3 (72
  tiles: split binning at the default), two L = 1 units (the first must equal
  wc_forward_tol's bytes), a unit without cells, a constant box, the
  wide-range 32x16x12 Gaussian x 1e30 at L2, and the NaN / inf specials of
  modes_batches at 8^3 L2."""
import math

import numpy as np
import pytest

import coarse_ref as C
import leveltol_rule as LT
import levels_ref as R
import modes_batches as M
from test_gpu_fuzz import _OPTION_SETS, same_cells
from test_gpu_modes_fuzz import LOOKBACK, options
from tol_rule import MARGIN, field, same_bits
from wavelet_compression_amd.capi import WC_MAX_LEVELS, WC_OPT_HOST_CHUNK, WC_OPT_TOL_SOLO_TILES

pytestmark = pytest.mark.gpu

# (dims, L, what): what = a tol_rule.field kind, or a tag
SPEC = [((4, 4, 4), 2, 0), ((8, 8, 8), 3, 1), ((16, 16, 16), 4, 2), ((12, 20, 8), 2, 0), ((48, 16, 80), 4, 0),
        ((64, 64, 64), 3, 2), ((64, 64, 72), 3, 0), ((16, 16, 24), 1, 0), ((4, 2, 6), 1, 1), ((0, 8, 8), 2, "empty"),
        ((16, 16, 16), 3, 3), (M.TOL_WIDE[1], 2, "wide")] + [(d, L, t) for t, d, L in M.SPECIALS]
ONE_LEVEL = 7  # the L = 1 unit compared with wc_forward_tol
# Per unit: 0.0, +inf, or the exponent u of 10^u times the unit's RMS (the set modes_batches.tol_batch
# draws from), fixed here so that the units that take a path of their own get a binding tolerance.
TOL_OF = [-1.0, 0.0, -2.0, math.inf, -1.5, -1.0, -2.5, -1.0, -0.5, -1.0, -3.0, "rms", -1.0, math.inf, -2.0]
assert len(TOL_OF) == len(SPEC)
SENT_T, SENT_B = -7.0, -7.0


class Case:
    """The batch in one cell type with its reference results, computed once and left unchanged."""

    def __init__(self, wc, oracle, dtype):
        rng = np.random.default_rng(8100)
        self.dtype = dtype
        self.dims = [d for d, _, _ in SPEC]
        self.levels = [L for _, L, _ in SPEC]
        self.n = len(SPEC)
        self.units, _, self.extent = wc.capi.make_units(self.dims)
        self.cells = np.zeros(self.extent, dtype)
        self.boxes, self.tol, self.finite = [], [], []
        for i, ((W, H, D), L, what) in enumerate(SPEC):
            if what == "empty":
                b = np.zeros((D, H, W), np.float64)
            elif what == "wide":
                b = rng.standard_normal((D, H, W)) * 1e30
            elif isinstance(what, str):
                b = M.special_box(what, (W, H, D), rng)
            else:
                b = field(what, W, H, D, seed=60 + i).astype(np.float64)
            o = self.units[i].cell_offset
            self.cells[o:o + b.size] = b.ravel().astype(dtype)
            b32 = M.narrow(oracle, b, dtype)
            self.boxes.append(b32)
            self.finite.append(bool(np.isfinite(b32).all()))
            f = b32.astype(np.float64)
            f = f[np.isfinite(f)]
            rms = float(np.sqrt(np.mean(f * f))) if f.size else 0.0
            u = TOL_OF[i]
            # "rms": the wide-range unit at its own RMS, the rule's S is about 10^60 N
            self.tol.append(rms if u == "rms" else u if u in (0.0, math.inf) else 10.0 ** u * rms)
        kinds = {0.0: "zero", math.inf: "inf"}
        assert {kinds.get(t, "finite") for t in self.tol} == {"zero", "inf", "finite"}
        self.owned = np.zeros(self.extent, bool)
        self.want = []  # (payload, kept, [thresh_l], bound)
        self.regen = []
        for i, b in enumerate(self.boxes):
            o = self.units[i].cell_offset
            self.owned[o:o + b.size] = True
            pay, kept, th, bd, _, _ = LT.payload(b, self.levels[i], self.tol[i])
            self.want.append((pay, kept, th, bd))
            self.regen.append(R.decode(pay)[0])


_cases = {}


@pytest.fixture(scope="module")
def case(wc, oracle):
    def get(dtype):
        if dtype not in _cases:
            _cases[dtype] = Case(wc, oracle, dtype)
        return _cases[dtype]
    return get


class Dev:
    """Device buffers of one batch, prefilled with sentinels."""

    def __init__(self, wc, B, units=None, n=None, cells=None):
        import torch
        dev = torch.device("cuda", 0)
        self.wc = wc
        self.units, self.n = (B.units, B.n) if units is None else (units, n)
        cells = B.cells if cells is None else cells
        self.code = wc.capi.WC_F64 if cells.dtype == np.float64 else wc.capi.WC_F32
        self.cells = torch.from_numpy(cells).to(dev)
        self.cap = wc.capi.payload_bound(self.units, self.n)
        self.pay = torch.full((self.cap,), 0xA5, dtype=torch.uint8, device=dev)
        self.off = torch.full((self.n + 1,), -3, dtype=torch.int64, device=dev)
        self.kept = torch.full((self.n,), -1, dtype=torch.int32, device=dev)
        self.thresh = torch.full((self.n, WC_MAX_LEVELS), SENT_T, dtype=torch.float32, device=dev)
        self.bound = torch.full((self.n,), SENT_B, dtype=torch.float64, device=dev)
        self.out = torch.full((max(int(cells.size), 1),), -77.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()  # the fills run on torch's stream, the context on its own

    def out_args(self, nulls=False):
        a = (self.pay.data_ptr(), self.cap, self.off.data_ptr(), self.kept.data_ptr())
        return a if nulls else a + (self.thresh.data_ptr(), self.bound.data_ptr())

    def read(self):
        pay = self.pay.cpu().numpy()
        off = self.off.cpu().numpy().view(np.uint64)
        kept = self.kept.cpu().numpy().view(np.uint32)
        payloads = [self.wc.capi.unit_payload(pay, off, kept, i) for i in range(self.n)]
        return payloads, kept.copy(), off.copy(), self.thresh.cpu().numpy(), self.bound.cpu().numpy()

    def untouched(self):
        return (bool((self.pay == 0xA5).all()) and bool((self.off == -3).all()) and bool((self.kept == -1).all())
                and bool((self.thresh == SENT_T).all()) and bool((self.bound == SENT_B).all())
                and bool((self.out == -77.0).all()))


def check_outputs(B, got, what, thresholds=True):
    payloads, kept, off, thresh, bound = got
    slot = 4
    for i in range(B.n):
        pay, k, th, bd = B.want[i]
        who = (what, i, B.dims[i], B.levels[i], B.tol[i])
        if thresholds:
            for l in range(WC_MAX_LEVELS):
                want = th[l] if l < B.levels[i] else 0.0
                assert same_bits(float(thresh[i, l]), want, np.float32), (who, l + 1, float(thresh[i, l]), want)
            assert same_bits(float(bound[i]), bd), (who, float(bound[i]), bd)
            assert bound[i] <= B.tol[i]
        assert int(kept[i]) == k, (who, int(kept[i]), k)
        assert payloads[i] == pay, who
        assert int(off[i]) == slot, who  # the slot rule of wc_forward
        slot += 24 + 8 * B.boxes[i].size
    assert int(off[B.n]) == int(off[B.n - 1]) + 20 + 8 * int(kept[B.n - 1])


def forward(wc, ctx, B, nulls=False):
    d = Dev(wc, B)
    ctx.forward_levels_tol(d.cells.data_ptr(), d.code, B.units, B.n, B.levels, B.tol, *d.out_args(nulls))
    ctx.synchronize()
    return d


def check_regen(ctx, B, d, what):
    """The payloads on the device through wc_inverse_levels against levels_ref.decode."""
    ctx.inverse_levels(d.pay.data_ptr(), d.off.data_ptr(), B.units, B.n, B.levels, d.out.data_ptr())
    ctx.synchronize()
    out = d.out.cpu().numpy()
    for i, b in enumerate(B.boxes):
        o = B.units[i].cell_offset
        assert same_cells(out[o:o + b.size], B.regen[i].ravel()), (what, i, B.dims[i], B.levels[i])
    assert np.all(out[~B.owned] == -77.0), (what, "written outside the units")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mixed_batch_matches_the_restatement(wc, ctx, case, dtype):
    B = case(dtype)
    solo = ctx.get_option(WC_OPT_TOL_SOLO_TILES)
    tiles = [-(-b.size // 4096) for b in B.boxes]
    assert solo == 64 and max(tiles) > solo and solo in tiles  # both binning paths, and the solo limit itself
    d = forward(wc, ctx, B)
    check_outputs(B, d.read(), ("default", dtype.__name__))
    check_regen(ctx, B, d, ("default", dtype.__name__))
    # the L = 1 unit alone through wc_forward_tol: the same bytes, threshold and bound
    i = ONE_LEVEL
    assert B.levels[i] == 1 and B.boxes[i].size
    units, n, extent = wc.capi.make_units([B.dims[i]])
    one = Dev(wc, B, units, n, B.boxes[i].ravel().astype(dtype))
    ctx.forward_tol(one.cells.data_ptr(), one.code, units, n, [B.tol[i]], one.pay.data_ptr(), one.cap,
                    one.off.data_ptr(), one.kept.data_ptr(), one.thresh.data_ptr(), one.bound.data_ptr())
    ctx.synchronize()
    pays, kept, _, thresh, bound = one.read()
    assert pays[0] == B.want[i][0] and int(kept[0]) == B.want[i][1]
    assert same_bits(float(thresh.ravel()[0]), B.want[i][2][0], np.float32) and same_bits(float(bound[0]), B.want[i][3])


@pytest.mark.parametrize("opts", ["solo_tiles_1", *LOOKBACK])
def test_option_sets(wc, ctx, case, opts):
    """Every unit of two or more tiles split (WC_OPT_TOL_SOLO_TILES = 1), and the
    look-back forms of the emit: the same outputs."""
    pairs = ((WC_OPT_TOL_SOLO_TILES, 1),) if opts == "solo_tiles_1" else _OPTION_SETS[opts]
    for dtype in (np.float32, np.float64):
        B = case(dtype)
        with options(wc, ctx, pairs):
            d = forward(wc, ctx, B)
        check_outputs(B, d.read(), (opts, dtype.__name__))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("chunk", [None, 3000])
def test_host_form(wc, ctx, oracle, case, dtype, chunk):
    """wc_forward_levels_tol_host in one run and in several: the device call's
    payloads, packed; thresholds and bounds; rmse = the RMSE of the reference
    reconstruction (the summation-order bound of test_gpu_fuzz.py), within the
    tolerance on the finite units with tol >= 1e-3."""
    B = case(dtype)
    with options(wc, ctx, ((WC_OPT_HOST_CHUNK, chunk),) if chunk is not None else ()):
        payload, offs, kept, thresh, bound, rmse = ctx.forward_levels_tol_host(B.cells, B.units, B.n, B.levels, B.tol)
    pos = 4
    for i in range(B.n):
        pay, k, th, bd = B.want[i]
        assert int(kept[i]) == k and int(offs[i]) == pos, i  # packed as wc_forward_host: 24 + 8 * kept apart
        assert wc.capi.unit_payload(payload, offs, kept, i) == pay, i
        pos += 24 + 8 * k
        for l in range(WC_MAX_LEVELS):
            assert same_bits(float(thresh[i, l]), th[l] if l < B.levels[i] else 0.0, np.float32), (i, l + 1)
        assert same_bits(float(bound[i]), bd), i
        if not B.boxes[i].size:
            assert rmse[i] == 0.0
            continue
        ref = oracle.rmse(B.boxes[i], B.regen[i])
        print(f"unit {i} dims {B.dims[i]} L {B.levels[i]} tol {B.tol[i]:g} kept {k} bound {bound[i]:.6g} "
              f"rmse {rmse[i]:.6g}")
        if np.isnan(ref):
            assert np.isnan(rmse[i]), (i, rmse[i])
        elif np.isinf(ref):
            assert rmse[i] == ref, (i, rmse[i], ref)
        else:
            assert abs(rmse[i] - ref) <= max(1e-12, (B.boxes[i].size + 4) * 2.0 ** -53) * abs(ref), (i, rmse[i], ref)
        if B.finite[i] and B.tol[i] >= 1e-3:
            assert rmse[i] <= B.tol[i] * (1 + MARGIN), (i, B.dims[i], B.tol[i], rmse[i])
    assert int(offs[B.n]) == pos - 4


def test_null_thresh_and_bound(wc, ctx, case):
    B = case(np.float32)
    d = forward(wc, ctx, B, nulls=True)
    got = d.read()
    check_outputs(B, got, "nulls", thresholds=False)
    assert (got[3] == SENT_T).all() and (got[4] == SENT_B).all()
    # one of the two
    d = Dev(wc, B)
    ctx.forward_levels_tol(d.cells.data_ptr(), d.code, B.units, B.n, B.levels, B.tol, *d.out_args(True), None,
                           d.bound.data_ptr())
    ctx.synchronize()
    got = d.read()
    check_outputs(B, got, "null thresh", thresholds=False)
    assert (got[3] == SENT_T).all() and all(same_bits(float(got[4][i]), B.want[i][3]) for i in range(B.n))


def test_coarse_decode_of_the_payloads(wc, ctx, case):
    """The format does not change: wc_inverse_coarse at r = 1 reads these payloads."""
    import torch
    B = case(np.float64)
    d = forward(wc, ctx, B)
    reduce = [1 if b.size else 0 for b in B.boxes]
    out_units, extent = wc.capi.coarse_units(B.units, B.n, reduce)
    out = torch.full((max(extent, 1),), -77.0, dtype=torch.float32, device=d.pay.device)
    torch.cuda.synchronize()
    ctx.inverse_coarse(d.pay.data_ptr(), d.off.data_ptr(), B.units, B.n, B.levels, reduce, out_units, out.data_ptr())
    ctx.synchronize()
    got = out.cpu().numpy()
    for i in range(B.n):
        want = C.decode(B.want[i][0], reduce[i]).ravel()
        o = out_units[i].cell_offset
        assert same_cells(got[o:o + want.size], want), (i, B.dims[i], B.levels[i])


def test_refusals_leave_the_outputs_untouched(wc, ctx, case):
    dims = [(16, 16, 16), (12, 20, 8), (4, 6, 2), (0, 3, 5)]
    units, n, extent = wc.capi.make_units(dims)
    cells = np.ones(extent, np.float32)
    good_l, good_t = [3, 2, 1, 1], [0.1, 0.1, 0.1, 0.1]
    bad = [([5, 2, 1, 1], good_t, "unit 0", "levels"),             # outside 1..WC_MAX_LEVELS
           ([3, 0, 1, 1], good_t, "unit 1", "levels"),
           ([3, 3, 1, 1], good_t, "unit 1", "divisible by 8"),       # 12 and 20 are not
           ([3, 2, 2, 1], good_t, "unit 2", "divisible by 4"),
           (good_l, [0.1, -1.0, 0.1, 0.1], "unit 1", "tolerance"),
           (good_l, [0.1, 0.1, 0.1, math.nan], "unit 3", "tolerance")]
    odd = wc.capi.make_units([(16, 16, 16), (4, 3, 2)])
    d = Dev(wc, None, units, n, cells)
    for lv, tol, who, why in bad:
        for call in (lambda: ctx.forward_levels_tol(d.cells.data_ptr(), d.code, units, n, lv, tol, *d.out_args()),
                     lambda: ctx.forward_levels_tol_host(cells, units, n, lv, tol)):
            with pytest.raises(wc.WaveletError) as ei:
                call()
            assert ei.value.code == wc.capi.WC_ERR_INVALID and who in str(ei.value) and why in str(ei.value), str(ei.value)
    # a unit with cells, L = 1 and an odd dimension
    d2 = Dev(wc, None, odd[0], odd[1], np.ones(odd[2], np.float32))
    for call in (lambda: ctx.forward_levels_tol(d2.cells.data_ptr(), d2.code, odd[0], odd[1], [2, 1], 0.1, *d2.out_args()),
                 lambda: ctx.forward_levels_tol_host(np.ones(odd[2], np.float32), odd[0], odd[1], [2, 1], 0.1)):
        with pytest.raises(wc.WaveletError) as ei:
            call()
        assert ei.value.code == wc.capi.WC_ERR_INVALID and "unit 1" in str(ei.value) and "even" in str(ei.value)
    ctx.synchronize()
    assert d.untouched() and d2.untouched()  # nothing was launched
    # the context goes on
    ctx.forward_levels_tol(d.cells.data_ptr(), d.code, units, n, good_l, good_t, *d.out_args())
    ctx.synchronize()
    pays, kept, _, thresh, bound = d.read()
    for i, (W, H, D) in enumerate(dims):
        pay, k, th, bd, _, _ = LT.payload(np.ones((D, H, W), np.float32), good_l[i], good_t[i])
        assert pays[i] == pay and int(kept[i]) == k and same_bits(float(bound[i]), bd), i
    assert kept.tolist() == [8, 30, 6, 0]  # constant boxes: the low-pass corners


def test_nothing_is_left_staged(wc, ctx, case):
    B = case(np.float32)
    d = forward(wc, ctx, B)
    before = d.read()
    with pytest.raises(wc.WaveletError) as ei:
        ctx.forward_emit_tol(B.units, B.n, 0.1, d.pay.data_ptr(), d.cap, d.off.data_ptr(), d.kept.data_ptr())
    assert ei.value.code == wc.capi.WC_ERR_INVALID and "no staged coefficients" in str(ei.value)
    ctx.synchronize()
    after = d.read()
    assert before[0] == after[0] and all(a.tobytes() == b.tobytes() for a, b in zip(before[1:], after[1:]))


def test_codec_compress_payloads_with_rmse(wc, oracle):
    """codec.compress_payloads(levels=3, rmse=...) gives the restatement's bytes at
    the levels each box admits and round-trips through decompress_payloads
    within the tolerance."""
    from wavelet_compression_amd import codec
    boxes = [field(0, 16, 16, 16, seed=3), field(2, 32, 16, 48, seed=4), field(1, 12, 20, 8, seed=5),
             field(0, 6, 10, 14, seed=6)]
    tols = [0.05, 0.2, 1.0, 0.01]
    pays = codec.compress_payloads(boxes, keep=0.5, levels=3, rmse=tols)
    lv = [R.levels_for(*b.shape[::-1], 3) for b in boxes]
    assert lv == [3, 3, 2, 1]
    for p, b, L, t in zip(pays, boxes, lv, tols):
        assert p == LT.payload(b, L, t)[0]
        assert wc.capi.payload_levels(p[:20]) == L
    same = codec.compress_payloads(boxes, keep=0.5, levels=3, rmse=0.2)
    assert same[1] == pays[1]
    for r, b, t in zip(codec.decompress_payloads(pays), boxes, tols):
        assert r.shape == b.shape
        assert oracle.rmse(b, r) <= t * (1 + MARGIN), (b.shape, t)
    # rmse=None is the keep rule, as before
    assert codec.compress_payloads(boxes[:1], keep=0.999, levels=3)[0] == R.payload(boxes[0], 3, keep=0.999)[0]
