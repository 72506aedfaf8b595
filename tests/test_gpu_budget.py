"""GPU: the size-budget mode (include/wavelet_amd.h wc_forward_levels_budget /
wc_forward_levels_budget_host) against the numpy restatement of the rule
(budget_rule.py) on levels_ref's final arrays.

Bar: per unit, the device's T and per-level thresholds equal the rule's bit for
bit (entries past the unit's L are 0.0f); the payload bytes equal the oracle's
RLE + serialize of exactly the candidates with key > T; the kept count equals
the restatement's and is <= K; slot offsets follow; the reconstruction through
wc_inverse_levels equals levels_ref.decode of those bytes
(test_gpu_fuzz.same_cells); an L = 1 payload decodes through plain wc_inverse;
the solo and split paths of the select and every look-back form of the emit give
the same outputs.

The batch and its budgets are budget_rule.Batch's: CALLS calls over one mixed
batch in fp32 and in fp64 cells, every unit with another class of budget in
every call (test_budget_cpu.py proves on the CPU that every class occurs and
that each chosen K has the property its class names)."""
import numpy as np
import pytest

import budget_rule as BR
import levels_ref as R
from test_gpu_fuzz import _OPTION_SETS, same_cells
from test_gpu_modes_fuzz import LOOKBACK, options
from tol_rule import field, same_bits
from wavelet_compression_amd.capi import WC_MAX_LEVELS, WC_OPT_HOST_CHUNK, WC_OPT_TOL_SOLO_TILES

pytestmark = pytest.mark.gpu

SENT_T, SENT_K = -7.0, 0x5A5A5A5A
_cases = {}


@pytest.fixture(scope="module")
def case(wc, oracle):
    def get(dtype):
        if dtype not in _cases:
            _cases[dtype] = BR.Batch(wc.capi, dtype)
        return _cases[dtype]
    return get


class Dev:
    """Device buffers of one batch, prefilled with sentinels."""

    def __init__(self, wc, units, n, cells):
        import torch
        dev = torch.device("cuda", 0)
        self.wc, self.units, self.n = wc, units, n
        self.code = wc.capi.WC_F64 if cells.dtype == np.float64 else wc.capi.WC_F32
        self.cells = torch.from_numpy(cells).to(dev)
        self.cap = wc.capi.payload_bound(units, n)
        self.pay = torch.full((self.cap,), 0xA5, dtype=torch.uint8, device=dev)
        self.off = torch.full((n + 1,), -3, dtype=torch.int64, device=dev)
        self.kept = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.thresh = torch.full((n, WC_MAX_LEVELS), SENT_T, dtype=torch.float32, device=dev)
        self.key = torch.full((n,), SENT_K, dtype=torch.int32, device=dev)
        self.out = torch.full((max(int(cells.size), 1),), -77.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()  # the fills run on torch's stream, the context on its own

    def out_args(self, nulls=False):
        a = (self.pay.data_ptr(), self.cap, self.off.data_ptr(), self.kept.data_ptr())
        return a if nulls else a + (self.thresh.data_ptr(), self.key.data_ptr())

    def read(self):
        pay = self.pay.cpu().numpy()
        off = self.off.cpu().numpy().view(np.uint64)
        kept = self.kept.cpu().numpy().view(np.uint32)
        payloads = [self.wc.capi.unit_payload(pay, off, kept, i) for i in range(self.n)]
        return payloads, kept.copy(), off.copy(), self.thresh.cpu().numpy(), self.key.cpu().numpy().view(np.uint32)

    def untouched(self):
        return (bool((self.pay == 0xA5).all()) and bool((self.off == -3).all()) and bool((self.kept == -1).all())
                and bool((self.thresh == SENT_T).all()) and bool((self.key == SENT_K).all())
                and bool((self.out == -77.0).all()))


def check_outputs(B, j, got, what, selection=True):
    payloads, kept, off, thresh, key = got
    slot = 4
    for i in range(B.n):
        pay, k, T, th, _ = B.want[j][i]
        K = B.budgets[j][i]
        who = (what, j, i, B.dims[i], B.levels[i], B.shown[j][i], K)
        if selection:
            assert int(key[i]) == T, (who, hex(int(key[i])), hex(T))
            for l in range(WC_MAX_LEVELS):
                want = th[l] if l < B.levels[i] else 0.0
                assert same_bits(float(thresh[i, l]), want, np.float32), (who, l + 1, float(thresh[i, l]), want)
        assert int(kept[i]) == k and k <= K, (who, int(kept[i]), k)
        assert payloads[i] == pay, who
        assert int(off[i]) == slot, who  # the slot rule of wc_forward
        slot += 24 + 8 * B.boxes[i].size
    assert int(off[B.n]) == int(off[B.n - 1]) + 20 + 8 * int(kept[B.n - 1])


def forward(wc, ctx, B, j, nulls=False):
    d = Dev(wc, B.units, B.n, B.cells)
    ctx.forward_levels_budget(d.cells.data_ptr(), d.code, B.units, B.n, B.levels, B.budgets[j], *d.out_args(nulls))
    ctx.synchronize()
    return d


def check_regen(ctx, B, j, d, what):
    """The payloads on the device through wc_inverse_levels against levels_ref.decode."""
    ctx.inverse_levels(d.pay.data_ptr(), d.off.data_ptr(), B.units, B.n, B.levels, d.out.data_ptr())
    ctx.synchronize()
    out = d.out.cpu().numpy()
    for i, b in enumerate(B.boxes):
        o = B.units[i].cell_offset
        assert same_cells(out[o:o + b.size], B.regen[j][i].ravel()), (what, j, i, B.dims[i], B.levels[i])
    assert np.all(out[~B.owned] == -77.0), (what, "written outside the units")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mixed_batch_matches_the_restatement(wc, ctx, case, dtype):
    B = case(dtype)
    solo = ctx.get_option(WC_OPT_TOL_SOLO_TILES)
    tiles = [-(-b.size // 4096) for b in B.boxes]
    assert solo == 64 and max(tiles) > solo and solo in tiles  # both paths of the select, and the solo limit itself
    for j in range(BR.CALLS):
        d = forward(wc, ctx, B, j)
        check_outputs(B, j, d.read(), ("default", dtype.__name__))
        check_regen(ctx, B, j, d, ("default", dtype.__name__))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_level_payloads_decode_through_plain_inverse(wc, ctx, case, dtype):
    """The L = 1 unit alone: the same bytes, and wc_inverse (the reference's format) reads them."""
    B = case(dtype)
    i = BR.ONE_LEVEL
    units, n, _ = wc.capi.make_units([B.dims[i]])
    for j in range(BR.CALLS):
        one = Dev(wc, units, n, B.boxes[i].ravel().astype(dtype))
        ctx.forward_levels_budget(one.cells.data_ptr(), one.code, units, n, None, [B.budgets[j][i]], *one.out_args())
        ctx.synchronize()
        pays, kept, _, thresh, key = one.read()
        assert pays[0] == B.want[j][i][0] and int(kept[0]) == B.want[j][i][1] and int(key[0]) == B.want[j][i][2], j
        assert thresh[0, 1:].tolist() == [0.0] * (WC_MAX_LEVELS - 1)
        ctx.inverse(one.pay.data_ptr(), one.off.data_ptr(), units, n, one.out.data_ptr())
        ctx.synchronize()
        assert same_cells(one.out.cpu().numpy()[:B.boxes[i].size], B.regen[j][i].ravel()), j


@pytest.mark.parametrize("opts", ["solo_tiles_1", *LOOKBACK])
def test_option_sets(wc, ctx, case, opts):
    """Every unit of two or more tiles split (WC_OPT_TOL_SOLO_TILES = 1), and the
    look-back forms of the emit: the same outputs."""
    pairs = ((WC_OPT_TOL_SOLO_TILES, 1),) if opts == "solo_tiles_1" else _OPTION_SETS[opts]
    for dtype in (np.float32, np.float64):
        B = case(dtype)
        for j in range(BR.CALLS):
            with options(wc, ctx, pairs):
                d = forward(wc, ctx, B, j)
            check_outputs(B, j, d.read(), (opts, dtype.__name__))


def test_null_thresh_and_key(wc, ctx, case):
    B = case(np.float32)
    for j in (1, 4):
        d = forward(wc, ctx, B, j, nulls=True)
        got = d.read()
        check_outputs(B, j, got, "nulls", selection=False)
        assert (got[3] == SENT_T).all() and (got[4] == SENT_K).all()
    # one of the two, with every unit split as well
    for pairs in ((), ((WC_OPT_TOL_SOLO_TILES, 1),)):
        d = Dev(wc, B.units, B.n, B.cells)
        with options(wc, ctx, pairs):
            ctx.forward_levels_budget(d.cells.data_ptr(), d.code, B.units, B.n, B.levels, B.budgets[2], *d.out_args(True),
                                      None, d.key.data_ptr())
            ctx.synchronize()
        got = d.read()
        check_outputs(B, 2, got, "null thresh", selection=False)
        assert (got[3] == SENT_T).all() and [int(k) for k in got[4]] == [w[2] for w in B.want[2]]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("chunk", [None, 3000])
def test_host_form(wc, ctx, oracle, case, dtype, chunk):
    """wc_forward_levels_budget_host in one run and in several: the device call's
    payloads, packed; thresholds and keys; rmse = the RMSE of the reference
    reconstruction (the summation-order bound of test_gpu_leveltol.py's host
    test).  The host arrays of levels and budgets are consumed by each device
    call before it returns: the host form hands every run its own slice."""
    B = case(dtype)
    j = 3
    with options(wc, ctx, ((WC_OPT_HOST_CHUNK, chunk),) if chunk is not None else ()):
        payload, offs, kept, thresh, key, rmse = ctx.forward_levels_budget_host(B.cells, B.units, B.n, B.levels,
                                                                               B.budgets[j])
    pos = 4
    for i in range(B.n):
        pay, k, T, th, _ = B.want[j][i]
        assert int(kept[i]) == k and int(offs[i]) == pos, i  # packed as wc_forward_host: 24 + 8 * kept apart
        assert wc.capi.unit_payload(payload, offs, kept, i) == pay, i
        pos += 24 + 8 * k
        assert int(key[i]) == T, i
        for l in range(WC_MAX_LEVELS):
            assert same_bits(float(thresh[i, l]), th[l] if l < B.levels[i] else 0.0, np.float32), (i, l + 1)
        if not B.boxes[i].size:
            assert rmse[i] == 0.0
            continue
        ref = oracle.rmse(B.boxes[i], B.regen[j][i])
        print(f"unit {i} dims {B.dims[i]} L {B.levels[i]} K {B.budgets[j][i]} kept {k} rmse {rmse[i]:.6g}")
        if np.isnan(ref):
            assert np.isnan(rmse[i]), (i, rmse[i])
        elif np.isinf(ref):
            assert rmse[i] == ref, (i, rmse[i], ref)
        else:
            assert abs(rmse[i] - ref) <= max(1e-12, (B.boxes[i].size + 4) * 2.0 ** -53) * abs(ref), (i, rmse[i], ref)
    assert int(offs[B.n]) == pos - 4
    # without rmse: no round trip, the same bytes
    with options(wc, ctx, ((WC_OPT_HOST_CHUNK, chunk),) if chunk is not None else ()):
        p2, o2, k2, _, _, none = ctx.forward_levels_budget_host(B.cells, B.units, B.n, B.levels, B.budgets[j],
                                                               want_rmse=False)
    assert none is None and o2.tolist() == offs.tolist() and k2.tolist() == kept.tolist()
    for i in range(B.n):  # (the four bytes between two packed payloads are not written)
        assert wc.capi.unit_payload(p2, o2, k2, i) == B.want[j][i][0], i


def test_host_arrays_are_consumed_before_the_call_returns(wc, ctx, case):
    """levels and max_pairs are overwritten right after the device call returns, before anything is
    synchronized: no effect."""
    B = case(np.float32)
    j = 5
    d = Dev(wc, B.units, B.n, B.cells)
    lv = np.array(B.levels, np.int32)
    mp = np.array(B.budgets[j], np.uint32)
    L = wc.capi.load_library()
    import ctypes
    rc = L.wc_forward_levels_budget(ctx.handle, ctypes.c_void_p(d.cells.data_ptr()), d.code, B.units, B.n,
                                    lv.ctypes.data, mp.ctypes.data, ctypes.c_void_p(d.pay.data_ptr()), d.cap,
                                    ctypes.c_void_p(d.off.data_ptr()), ctypes.c_void_p(d.kept.data_ptr()),
                                    ctypes.c_void_p(d.thresh.data_ptr()), ctypes.c_void_p(d.key.data_ptr()))
    lv[:] = 77
    mp[:] = 1
    assert rc == 0
    ctx.synchronize()
    check_outputs(B, j, d.read(), "overwritten host arrays")


def test_refusals_leave_the_outputs_untouched(wc, ctx):
    dims = [(16, 16, 16), (12, 20, 8), (4, 6, 2), (0, 3, 5)]
    units, n, extent = wc.capi.make_units(dims)
    cells = np.ones(extent, np.float32)
    good_l, good_k = [3, 2, 1, 1], [5, 1000, 2, 9]
    bad = [([5, 2, 1, 1], "unit 0", "levels"),             # outside 1..WC_MAX_LEVELS
           ([3, 0, 1, 1], "unit 1", "levels"),
           ([3, 3, 1, 1], "unit 1", "divisible by 8"),       # 12 and 20 are not
           ([3, 2, 2, 1], "unit 2", "divisible by 4")]
    odd = wc.capi.make_units([(16, 16, 16), (4, 3, 2)])
    d = Dev(wc, units, n, cells)
    for lv, who, why in bad:
        for call in (lambda: ctx.forward_levels_budget(d.cells.data_ptr(), d.code, units, n, lv, good_k, *d.out_args()),
                     lambda: ctx.forward_levels_budget_host(cells, units, n, lv, good_k)):
            with pytest.raises(wc.WaveletError) as ei:
                call()
            assert ei.value.code == wc.capi.WC_ERR_INVALID and who in str(ei.value) and why in str(ei.value), str(ei.value)
    # a unit with cells, L = 1 and an odd dimension (levels NULL = all 1 as well)
    d2 = Dev(wc, odd[0], odd[1], np.ones(odd[2], np.float32))
    for lv in ([2, 1], None):
        for call in (lambda: ctx.forward_levels_budget(d2.cells.data_ptr(), d2.code, odd[0], odd[1], lv, 3, *d2.out_args()),
                     lambda: ctx.forward_levels_budget_host(np.ones(odd[2], np.float32), odd[0], odd[1], lv, 3)):
            with pytest.raises(wc.WaveletError) as ei:
                call()
            assert ei.value.code == wc.capi.WC_ERR_INVALID and "unit 1" in str(ei.value) and "even" in str(ei.value)
    # a null required buffer: cells, payload, offsets, kept, max_pairs
    import ctypes
    L = wc.capi.load_library()
    lv = np.array(good_l, np.int32)
    mp = np.array(good_k, np.uint32)
    ptrs = [d.cells.data_ptr(), lv.ctypes.data, mp.ctypes.data, d.pay.data_ptr(), d.off.data_ptr(), d.kept.data_ptr()]
    for null in (0, 2, 3, 4, 5):
        p = [ctypes.c_void_p(0 if q == null else v) for q, v in enumerate(ptrs)]
        rc = L.wc_forward_levels_budget(ctx.handle, p[0], d.code, units, n, p[1], p[2], p[3], d.cap, p[4], p[5],
                                        ctypes.c_void_p(d.thresh.data_ptr()), ctypes.c_void_p(d.key.data_ptr()))
        assert rc == wc.capi.WC_ERR_INVALID, null
    ctx.synchronize()
    assert d.untouched() and d2.untouched()  # nothing was launched
    # the context goes on
    ctx.forward_levels_budget(d.cells.data_ptr(), d.code, units, n, good_l, good_k, *d.out_args())
    ctx.synchronize()
    pays, kept, _, thresh, key = d.read()
    for i, (W, H, D) in enumerate(dims):
        pay, k, T, th, _ = BR.payload(np.ones((D, H, W), np.float32), good_l[i], good_k[i])
        assert pays[i] == pay and int(kept[i]) == k and int(key[i]) == T, i
    # constant boxes: the low-pass corners (8, 30, 6 candidates, all ties): a budget below that keeps nothing
    assert kept.tolist() == [0, 30, 0, 0]


def test_nothing_is_left_staged(wc, ctx, case):
    B = case(np.float32)
    d = forward(wc, ctx, B, 0)
    before = d.read()
    with pytest.raises(wc.WaveletError) as ei:
        ctx.forward_emit_tol(B.units, B.n, 0.1, d.pay.data_ptr(), d.cap, d.off.data_ptr(), d.kept.data_ptr())
    assert ei.value.code == wc.capi.WC_ERR_INVALID and "no staged coefficients" in str(ei.value)
    ctx.synchronize()
    after = d.read()
    assert before[0] == after[0] and all(a.tobytes() == b.tobytes() for a, b in zip(before[1:], after[1:]))


def test_codec_compress_payloads_under_a_budget(wc, oracle):
    """codec.compress_payloads(max_bytes= / ratio=): every payload within its byte bound and equal to the
    restatement's at the levels each box admits; the three size / quality controls exclude each other."""
    from wavelet_compression_amd import codec
    boxes = [field(0, 16, 16, 16, seed=3), field(2, 32, 16, 48, seed=4), field(1, 12, 20, 8, seed=5),
             field(0, 6, 10, 14, seed=6)]
    lv = [R.levels_for(*b.shape[::-1], 3) for b in boxes]
    assert lv == [3, 3, 2, 1]
    limits = [20, 1000, 4093, 10 ** 9]
    pays = codec.compress_payloads(boxes, keep=0.5, levels=3, max_bytes=limits)
    for p, b, L, m in zip(pays, boxes, lv, limits):
        assert len(p) <= m and p == BR.payload(b, L, (m - 20) // 8)[0]
        assert wc.capi.payload_levels(p[:20]) == L
    assert len(pays[0]) == 20
    same = codec.compress_payloads(boxes, keep=0.5, levels=3, max_bytes=1000)
    assert same[1] == pays[1] and all(len(p) <= 1000 for p in same)
    for ratio in (20, 7.5, 1e9):
        got = codec.compress_payloads(boxes, keep=0.5, levels=3, ratio=ratio)
        for p, b, L in zip(got, boxes, lv):
            m = max(20, int(4 * b.size / ratio))
            assert len(p) <= m and p == BR.payload(b, L, (m - 20) // 8)[0], (ratio, b.shape)
    for r, b in zip(codec.decompress_payloads(pays), boxes):
        assert r.shape == b.shape
    for kw in ({"rmse": 0.1, "ratio": 2}, {"rmse": 0.1, "max_bytes": 100}, {"max_bytes": 100, "ratio": 2}):
        with pytest.raises(ValueError):
            codec.compress_payloads(boxes, keep=0.5, levels=3, **kw)
    with pytest.raises(ValueError):
        codec.compress_payloads(boxes, keep=0.5, levels=3, max_bytes=19)
    with pytest.raises(ValueError):
        codec.compress_payloads(boxes, keep=0.5, levels=3, max_bytes=[100, 100])
