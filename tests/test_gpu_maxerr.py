"""GPU: the pointwise (max-abs) error bound (include/wavelet_amd.h
wc_forward_levels_maxerr / wc_forward_levels_maxerr_host / wc_maxerr,
codec.compress_payloads(levels=, maxerr=)) against the numpy restatement of the
rule (maxerr_rule.py) on levels_ref's final arrays.

Bar: per unit, the device's threshold and achieved error equal the rule's bit
for bit; the payload bytes equal levels_ref.payload at that threshold and what
wc_forward_levels writes for the unit alone at thresh = d_thresh[u]; kept counts
and slot offsets follow; the payloads decoded by wc_inverse_levels give, with
max|x - R| taken in numpy, exactly the d_err bits, which are <= E wherever the
threshold is above 0; wc_maxerr on those reconstructions gives the same bits
again; every look-back form of the emit and both solo / split settings give the
same outputs; the _host form gives the same bytes in one run and in runs of one
unit.

One mixed batch, in fp32 and in fp64 (unit: purpose):
  2x2x2 L1 (one block), 4x4x4 L2 twice (the box on which err(b) is not monotone:
  once in the bounds' cycle, once under E = 8 where the leading run stops at b* =
  2044 although b = 4095 passes), 8^3 L3, 16^3 L4, 12x20x8 L2, 48x16x80 L4 (the
  probe tiles do not divide the box), 64x64x72 L3 (many workgroups per unit: the
  atomics cross workgroups), a 2x2x4096 L1 pencil, a unit without cells, a
  constant box, the wide-range 32x16x12 Gaussian x 1e30 at L2, and the NaN / inf
  specials of modes_batches at 8^3 L2.  The fp64 cells differ from their fp32
  narrowing, so the error is taken against the cells before narrowing."""
import math

import numpy as np
import pytest

import levels_ref as R
import maxerr_rule as MR
import modes_batches as M
from test_gpu_fuzz import _OPTION_SETS
from test_gpu_modes_fuzz import LOOKBACK, options
from test_maxerr_cpu import nonmonotone_box
from tol_rule import field, same_bits
from wavelet_compression_amd.capi import WC_OPT_HOST_CHUNK, WC_OPT_TOL_SOLO_TILES

pytestmark = pytest.mark.gpu

# (dims, L, what): what = a tol_rule.field kind, or a tag
SPEC = [((2, 2, 2), 1, 1), ((4, 4, 4), 2, "nonmono"), ((4, 4, 4), 2, "nonmono"), ((8, 8, 8), 3, 1),
        ((16, 16, 16), 4, 2), ((12, 20, 8), 2, 0), ((48, 16, 80), 4, 0), ((64, 64, 72), 3, 0), ((2, 2, 4096), 1, 0),
        ((0, 8, 8), 2, "empty"), ((16, 16, 16), 3, 3), (M.TOL_WIDE[1], 2, "wide")] + [(d, L, t) for t, d, L in M.SPECIALS]
# Per unit: 0.0, +inf, an absolute bound ("abs", E), or the factor of the unit's max|x| over its finite cells.
# The cycle 0, +inf, 1e-9, 1e-1, 1e-2, 1e-3 runs twice over the batch, moved so that the units that take a
# path of their own get a binding bound.
BOUND_OF = [1e-1, 1e-2, ("abs", 8.0), 0.0, math.inf, 1e-9, 1e-1, 1e-2, 1e-3, 0.0, math.inf, 1e-9, 1e-1, 1e-2, 1e-3]
assert len(BOUND_OF) == len(SPEC)
SENT_T, SENT_E = -7.0, -7.0


class Case:
    """The batch in one cell type with its reference results, computed once and left unchanged."""

    def __init__(self, wc, oracle, dtype):
        rng = np.random.default_rng(9200)
        self.dtype = dtype
        self.dims = [d for d, _, _ in SPEC]
        self.levels = [L for _, L, _ in SPEC]
        self.n = len(SPEC)
        self.units, _, self.extent = wc.capi.make_units(self.dims)
        self.cells = np.zeros(self.extent, dtype)
        self.x, self.boxes, self.E = [], [], []
        for i, ((W, H, D), L, what) in enumerate(SPEC):
            if what == "empty":
                b = np.zeros((D, H, W), np.float64)
            elif what == "wide":
                b = rng.standard_normal((D, H, W)) * 1e30
            elif what == "nonmono":
                b = nonmonotone_box().astype(np.float64)
            elif isinstance(what, str):
                b = M.special_box(what, (W, H, D), rng)
            else:
                b = field(what, W, H, D, seed=90 + i).astype(np.float64)
                if dtype == np.float64 and what != 3:
                    b = b * (1.0 + 2.0 ** -30)  # not representable in fp32
            x = b.astype(dtype)
            o = self.units[i].cell_offset
            self.cells[o:o + x.size] = x.ravel()
            self.x.append(x)
            self.boxes.append(M.narrow(oracle, b, dtype))
            f = np.abs(x.astype(np.float64))
            f = f[np.isfinite(f)]
            m = float(f.max()) if f.size else 1.0
            u = BOUND_OF[i]
            self.E.append(u[1] if isinstance(u, tuple) else u if u in (0.0, math.inf) else u * m)
        self.owned = np.zeros(self.extent, bool)
        self.want = []  # (payload, kept, thresh, err, b*)
        for i, x in enumerate(self.x):
            o = self.units[i].cell_offset
            self.owned[o:o + x.size] = True
            self.want.append(MR.payload(x, self.levels[i], self.E[i], narrowed=self.boxes[i]))
        bs = [w[4] for w in self.want]
        # the classes the docstring claims
        assert self.want[2][4] == 2044 and self.want[2][3] == 6.75
        assert any(b == 0 and w[3] > E > 0 for b, w, E in zip(bs, self.want, self.E))  # accepted unverified
        assert any(0 < b < 4095 for b in bs) and 4095 in bs


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
        self.thresh = torch.full((self.n,), SENT_T, dtype=torch.float32, device=dev)
        self.err = torch.full((self.n,), SENT_E, dtype=torch.float64, device=dev)
        self.out = torch.full((max(int(cells.size), 1),), -77.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()  # the fills run on torch's stream, the context on its own

    def out_args(self, nulls=False):
        a = (self.pay.data_ptr(), self.cap, self.off.data_ptr(), self.kept.data_ptr())
        return a if nulls else a + (self.thresh.data_ptr(), self.err.data_ptr())

    def read(self):
        pay = self.pay.cpu().numpy()
        off = self.off.cpu().numpy().view(np.uint64)
        kept = self.kept.cpu().numpy().view(np.uint32)
        payloads = [self.wc.capi.unit_payload(pay, off, kept, i) for i in range(self.n)]
        return payloads, kept.copy(), off.copy(), self.thresh.cpu().numpy(), self.err.cpu().numpy()

    def untouched(self):
        return (bool((self.pay == 0xA5).all()) and bool((self.off == -3).all()) and bool((self.kept == -1).all())
                and bool((self.thresh == SENT_T).all()) and bool((self.err == SENT_E).all())
                and bool((self.out == -77.0).all()))


def check_outputs(B, got, what, selected=True):
    payloads, kept, off, thresh, err = got
    slot = 4
    for i in range(B.n):
        pay, k, th, e, b = B.want[i]
        who = (what, i, B.dims[i], B.levels[i], B.E[i], b)
        if selected:
            print(f"{what} unit {i} {B.dims[i]} L {B.levels[i]} E {B.E[i]:g}: b* {b} thresh {float(thresh[i]):g} "
                  f"(want {float(th):g}) err {float(err[i]):.17g} (want {e:.17g}) kept {int(kept[i])} (want {k})")
            assert same_bits(float(thresh[i]), float(th), np.float32), who
            assert same_bits(float(err[i]), e), who
            assert thresh[i] == 0.0 or err[i] <= B.E[i], who
        assert int(kept[i]) == k, (who, int(kept[i]), k)
        assert payloads[i] == pay, who
        assert int(off[i]) == slot, who  # the slot rule of wc_forward
        slot += 24 + 8 * B.boxes[i].size
    assert int(off[B.n]) == int(off[B.n - 1]) + 20 + 8 * int(kept[B.n - 1])


def forward(wc, ctx, B, nulls=False):
    d = Dev(wc, B)
    ctx.forward_levels_maxerr(d.cells.data_ptr(), d.code, B.units, B.n, B.levels, B.E, *d.out_args(nulls))
    ctx.synchronize()
    return d


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mixed_batch_matches_the_restatement(wc, ctx, case, dtype):
    import torch
    B = case(dtype)
    d = forward(wc, ctx, B)
    got = d.read()
    check_outputs(B, got, ("default", dtype.__name__))
    payloads, kept, off, thresh, err = got
    # each unit alone through wc_forward_levels at thresh = d_thresh[u]: the same bytes
    for i in range(B.n):
        units, n, _ = wc.capi.make_units([B.dims[i]])
        one = Dev(wc, B, units, n, np.ascontiguousarray(B.x[i].ravel()) if B.x[i].size else np.zeros(1, dtype))
        ctx.forward_levels(one.cells.data_ptr(), one.code, units, n, [B.levels[i]], 0.5, float(thresh[i]),
                           one.pay.data_ptr(), one.cap, one.off.data_ptr(), one.kept.data_ptr())
        ctx.synchronize()
        p1, k1, _, _, _ = one.read()
        assert p1[0] == payloads[i] and int(k1[0]) == int(kept[i]), (i, B.dims[i])
    # the payloads through wc_inverse_levels: max|x - R| in numpy is d_err, bit for bit
    ctx.inverse_levels(d.pay.data_ptr(), d.off.data_ptr(), B.units, B.n, B.levels, d.out.data_ptr())
    ctx.synchronize()
    out = d.out.cpu().numpy()
    for i, x in enumerate(B.x):
        o = B.units[i].cell_offset
        e = MR.max_abs(x, out[o:o + x.size])
        assert same_bits(e, float(err[i])), (i, B.dims[i], e, float(err[i]))
        assert thresh[i] == 0.0 or e <= B.E[i], (i, e, B.E[i])
    assert np.all(out[~B.owned] == -77.0)
    # wc_maxerr on those reconstructions: the same bits again, on the device and through the host form
    again = torch.full((B.n,), SENT_E, dtype=torch.float64, device=d.pay.device)
    torch.cuda.synchronize()
    ctx.maxerr(d.cells.data_ptr(), d.code, d.out.data_ptr(), B.units, B.n, again.data_ptr())
    ctx.synchronize()
    assert again.cpu().numpy().tobytes() == err.tobytes()
    assert ctx.maxerr_host(B.cells, out, B.units, B.n).tobytes() == err.tobytes()


@pytest.mark.parametrize("maxl", [1, 2, 3])
def test_every_probe_kernel(wc, ctx, case, maxl):
    """The probe kernel is compiled for the call's largest L (the mixed batch runs
    the L = 4 form, whose tile is 16 x 16 x 32): the units of at most maxl levels
    alone run the 16 x 8 x 32 forms, in both cell types, to the same results."""
    for dtype in (np.float32, np.float64):
        B = case(dtype)
        pick = [i for i in range(B.n) if B.levels[i] <= maxl]
        assert max(B.levels[i] for i in pick) == maxl
        dims = [B.dims[i] for i in pick]
        units, n, extent = wc.capi.make_units(dims)
        cells = np.zeros(extent, dtype)
        for k, i in enumerate(pick):
            cells[units[k].cell_offset:units[k].cell_offset + B.x[i].size] = B.x[i].ravel()
        d = Dev(wc, B, units, n, cells)
        ctx.forward_levels_maxerr(d.cells.data_ptr(), d.code, units, n, [B.levels[i] for i in pick],
                                  [B.E[i] for i in pick], *d.out_args())
        ctx.synchronize()
        pays, kept, _, thresh, err = d.read()
        for k, i in enumerate(pick):
            pay, kk, th, e, b = B.want[i]
            who = (maxl, dtype.__name__, i, B.dims[i])
            assert same_bits(float(thresh[k]), float(th), np.float32) and same_bits(float(err[k]), e), who
            assert pays[k] == pay and int(kept[k]) == kk, who


@pytest.mark.parametrize("opts", ["solo_tiles_1", *LOOKBACK])
def test_option_sets(wc, ctx, case, opts):
    """Both solo / split settings and the look-back forms of the emit: the same outputs."""
    pairs = ((WC_OPT_TOL_SOLO_TILES, 1),) if opts == "solo_tiles_1" else _OPTION_SETS[opts]
    for dtype in (np.float32, np.float64):
        B = case(dtype)
        with options(wc, ctx, pairs):
            d = forward(wc, ctx, B)
        check_outputs(B, d.read(), (opts, dtype.__name__))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("chunk", [None, 1])
def test_host_form(wc, ctx, oracle, case, dtype, chunk):
    """wc_forward_levels_maxerr_host in one run and in runs of one unit: the device
    call's payloads, packed; thresholds and errors; rmse = the RMSE of the
    reference reconstruction (the summation-order bound of test_gpu_fuzz.py)."""
    B = case(dtype)
    with options(wc, ctx, ((WC_OPT_HOST_CHUNK, chunk),) if chunk is not None else ()):
        payload, offs, kept, thresh, err, rmse = ctx.forward_levels_maxerr_host(B.cells, B.units, B.n, B.levels, B.E)
    pos = 4
    for i in range(B.n):
        pay, k, th, e, b = B.want[i]
        assert int(kept[i]) == k and int(offs[i]) == pos, i  # packed as wc_forward_host: 24 + 8 * kept apart
        assert wc.capi.unit_payload(payload, offs, kept, i) == pay, i
        pos += 24 + 8 * k
        assert same_bits(float(thresh[i]), float(th), np.float32) and same_bits(float(err[i]), e), i
        if not B.boxes[i].size:
            assert rmse[i] == 0.0
            continue
        ref = oracle.rmse(B.boxes[i], R.decode(pay)[0])
        if np.isnan(ref):
            assert np.isnan(rmse[i]), (i, rmse[i])
        elif np.isinf(ref):
            assert rmse[i] == ref, (i, rmse[i], ref)
        else:
            assert abs(rmse[i] - ref) <= max(1e-12, (B.boxes[i].size + 4) * 2.0 ** -53) * abs(ref), (i, rmse[i], ref)
    assert int(offs[B.n]) == pos - 4


def test_null_thresh_and_err(wc, ctx, case):
    B = case(np.float32)
    d = forward(wc, ctx, B, nulls=True)
    got = d.read()
    check_outputs(B, got, "nulls", selected=False)
    assert (got[3] == SENT_T).all() and (got[4] == SENT_E).all()
    d = Dev(wc, B)
    ctx.forward_levels_maxerr(d.cells.data_ptr(), d.code, B.units, B.n, B.levels, B.E, *d.out_args(True), None,
                              d.err.data_ptr())
    ctx.synchronize()
    got = d.read()
    check_outputs(B, got, "null thresh", selected=False)
    assert (got[3] == SENT_T).all() and all(same_bits(float(got[4][i]), B.want[i][3]) for i in range(B.n))


def test_levels_none_is_one_level(wc, ctx):
    dims = [(8, 4, 6), (16, 16, 16)]
    units, n, extent = wc.capi.make_units(dims)
    cells = np.concatenate([field(1, *d, seed=5 + i).ravel() for i, d in enumerate(dims)])
    d = Dev(wc, None, units, n, cells)
    ctx.forward_levels_maxerr(d.cells.data_ptr(), d.code, units, n, None, 0.25, *d.out_args())
    ctx.synchronize()
    pays, kept, _, thresh, err = d.read()
    for i, (W, H, D) in enumerate(dims):
        x = cells[units[i].cell_offset:units[i].cell_offset + W * H * D].reshape(D, H, W)
        pay, k, th, e, b = MR.payload(x, 1, 0.25)
        assert pays[i] == pay and same_bits(float(thresh[i]), float(th), np.float32) and same_bits(float(err[i]), e)
        assert 0 < b and e <= 0.25


def test_refusals_leave_the_outputs_untouched(wc, ctx):
    dims = [(16, 16, 16), (12, 20, 8), (4, 6, 2), (0, 3, 5)]
    units, n, extent = wc.capi.make_units(dims)
    cells = np.ones(extent, np.float32)
    good_l, good_e = [3, 2, 1, 1], [0.1, 0.1, 0.1, 0.1]
    bad = [([5, 2, 1, 1], good_e, "unit 0", "levels"),             # outside 1..WC_MAX_LEVELS
           ([3, 0, 1, 1], good_e, "unit 1", "levels"),
           ([3, 3, 1, 1], good_e, "unit 1", "divisible by 8"),       # 12 and 20 are not
           ([3, 2, 2, 1], good_e, "unit 2", "divisible by 4"),
           (good_l, [0.1, -1.0, 0.1, 0.1], "unit 1", "bound"),
           (good_l, [0.1, 0.1, 0.1, math.nan], "unit 3", "bound")]
    odd = wc.capi.make_units([(16, 16, 16), (4, 3, 2)])
    d = Dev(wc, None, units, n, cells)
    for lv, E, who, why in bad:
        for call in (lambda: ctx.forward_levels_maxerr(d.cells.data_ptr(), d.code, units, n, lv, E, *d.out_args()),
                     lambda: ctx.forward_levels_maxerr_host(cells, units, n, lv, E)):
            with pytest.raises(wc.WaveletError) as ei:
                call()
            assert ei.value.code == wc.capi.WC_ERR_INVALID and who in str(ei.value) and why in str(ei.value), str(ei.value)
    # a unit with cells, L = 1 and an odd dimension
    d2 = Dev(wc, None, odd[0], odd[1], np.ones(odd[2], np.float32))
    for call in (lambda: ctx.forward_levels_maxerr(d2.cells.data_ptr(), d2.code, odd[0], odd[1], [2, 1], 0.1, *d2.out_args()),
                 lambda: ctx.forward_levels_maxerr_host(np.ones(odd[2], np.float32), odd[0], odd[1], [2, 1], 0.1)):
        with pytest.raises(wc.WaveletError) as ei:
            call()
        assert ei.value.code == wc.capi.WC_ERR_INVALID and "unit 1" in str(ei.value) and "even" in str(ei.value)
    ctx.synchronize()
    assert d.untouched() and d2.untouched()  # nothing was launched
    # the context goes on
    ctx.forward_levels_maxerr(d.cells.data_ptr(), d.code, units, n, good_l, good_e, *d.out_args())
    ctx.synchronize()
    pays, kept, _, thresh, err = d.read()
    for i, (W, H, D) in enumerate(dims):
        pay, k, th, e, b = MR.payload(np.ones((D, H, W), np.float32), good_l[i], good_e[i])
        assert pays[i] == pay and int(kept[i]) == k and same_bits(float(err[i]), e), i
    assert kept.tolist() == [8, 30, 6, 0]  # constant boxes: the low-pass corners, 1 > 0.1 is not dropped


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


def test_caller_stream_without_a_host_sync(wc, case):
    """On a torch stream s, after wc_set_stream(s): a delay, then the producer
    (cells.copy_), the call, the decode and the metric, a clone of every output
    and the overwrite of the originals, all enqueued without a host sync.  After
    s.synchronize() alone the clones hold the restatement's results."""
    import torch
    from test_gpu_async import DELAY_MS, NO_POWER
    B = case(np.float64)
    ctx = wc.capi.Context(0)
    s = torch.cuda.Stream()
    try:
        d = Dev(wc, B)
        real = d.cells.clone()
        again = torch.full((B.n,), SENT_E, dtype=torch.float64, device=d.pay.device)

        def enqueue():
            ctx.forward_levels_maxerr(d.cells.data_ptr(), d.code, B.units, B.n, B.levels, B.E, *d.out_args())
            ctx.inverse_levels(d.pay.data_ptr(), d.off.data_ptr(), B.units, B.n, B.levels, d.out.data_ptr())
            ctx.maxerr(d.cells.data_ptr(), d.code, d.out.data_ptr(), B.units, B.n, again.data_ptr())

        enqueue()  # warm: nothing afterwards builds a plan or grows a buffer
        ctx.synchronize()
        probe = 2_000_000
        torch.cuda._sleep(probe)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        b.synchronize()
        cycles = max(probe, int(probe * DELAY_MS / a.elapsed_time(b)))
        outs = (d.pay, d.off, d.kept, d.thresh, d.err, again)
        for t in outs:
            t.fill_(0)
        d.cells.zero_()
        torch.cuda.synchronize()
        ctx.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            d.cells.copy_(real)
            enqueue()
            clones = [t.clone() for t in outs]
            for t in outs:
                t.fill_(0)
            d.cells.fill_(float("nan"))
            busy = not s.query()
        assert busy, NO_POWER
        s.synchronize()  # the torch sync only
        d.pay, d.off, d.kept, d.thresh, d.err = clones[:5]
        got = d.read()
        check_outputs(B, got, "caller stream")
        assert clones[5].cpu().numpy().tobytes() == got[4].tobytes()
        ctx.synchronize()
    finally:
        ctx.set_stream(None)
        ctx.close()


def test_codec_compress_payloads_with_maxerr(wc):
    """codec.compress_payloads(levels=3, maxerr=...) gives the restatement's bytes at
    the levels each box admits and round-trips through decompress_payloads within
    the bound; pack= composes as with rmse=; the modes exclude each other."""
    from wavelet_compression_amd import codec
    boxes = [field(0, 16, 16, 16, seed=3), field(2, 32, 16, 48, seed=4), field(1, 12, 20, 8, seed=5),
             field(0, 6, 10, 14, seed=6)]
    bounds = [0.05, 0.2, 1.0, 0.01]
    pays = codec.compress_payloads(boxes, keep=0.5, levels=3, maxerr=bounds)
    lv = [R.levels_for(*b.shape[::-1], 3) for b in boxes]
    assert lv == [3, 3, 2, 1]
    for p, b, L, E in zip(pays, boxes, lv, bounds):
        assert p == MR.payload(b, L, E)[0]
        assert wc.capi.payload_levels(p[:20]) == L
    assert codec.compress_payloads(boxes, keep=0.5, levels=3, maxerr=0.2)[1] == pays[1]
    for r, b, E in zip(codec.decompress_payloads(pays), boxes, bounds):
        assert r.shape == b.shape
        assert MR.max_abs(b, r) <= E, (b.shape, E)
    # fp64 boxes: the bound holds against the cells before narrowing
    b64 = [b.astype(np.float64) * (1.0 + 2.0 ** -30) for b in boxes[:2]]
    p64 = codec.compress_payloads(b64, keep=0.5, levels=3, maxerr=[0.05, 0.2])
    for p, b, L, E in zip(p64, b64, lv, [0.05, 0.2]):
        assert p == MR.payload(b, L, E)[0]
    packed = codec.compress_payloads(boxes, keep=0.5, levels=3, maxerr=bounds, pack=3)
    assert packed == codec.pack_payloads(pays, 3)
    for kw in ({"rmse": 0.1}, {"max_bytes": 100}, {"ratio": 4.0}):
        with pytest.raises(ValueError):
            codec.compress_payloads(boxes, keep=0.5, levels=3, maxerr=0.1, **kw)
