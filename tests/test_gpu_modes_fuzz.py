"""GPU: seeded random batches (tests/modes_batches.py) through the opt-in modes:
the multi-level transform (wc_*_levels*), the reduced-resolution decode
(wc_inverse_coarse*), the RMSE-tolerance mode (wc_forward_tol*,
wc_forward_emit_tol) and the accumulating histogram of wc_forward_stage,
against their CPU restatements (levels_ref.py, coarse_ref.py, tol_rule.py, the
oracle), specials included: NaN, +-inf, -0 and subnormal cells, a NaN that the
pyramid carries to A[0], inf - inf made by a level pass, bins at +inf.
tests/test_modes_batches_cpu.py proves without a GPU that the batches hold
those cases.

One convention for every comparison here.  Payload bytes, kept counts, slot
offsets, thresholds and bounds: bit for bit (a payload never holds a NaN).
Flat arrays and cells: test_gpu_fuzz.same_cells (bit for bit, a NaN matching
any NaN: DESIGN.md "Numerics").  RMSE: the rule test_gpu_fuzz.py derives,
max(1e-12, (n + 4) 2^-53) relative, NaN where the oracle's is NaN, an infinity
equal.  Every unit is compared (a unit without cells by its header); output
buffers are prefilled with sentinels, and every element no unit owns must
still hold its sentinel afterwards."""
import os

import numpy as np
import pytest

import levels_ref as R
import modes_batches as M
from test_gpu_coarse import Case, run_device, run_host
from test_gpu_fuzz import _OPTION_SETS, _batch, same_cells
from test_gpu_levels import Batch, Dev
from test_gpu_tol import Dev as TolDev
from tol_rule import same_bits, tol_rule
from wavelet_compression_amd.capi import WC_OPT_HOST_CHUNK, WC_OPT_TOL_SOLO_TILES

pytestmark = pytest.mark.gpu

_N = int(os.environ.get("WC_FUZZ_SEEDS", "0"))
SENTINEL = -77.0  # test_gpu_levels.Dev's and test_gpu_coarse.Dev's fill of float outputs
LOOKBACK = ("tickets", "reversed_tiles", "spin_limit_1", "reversed_spin_1")
HOST_CHUNKS = (0, 1 << 14, 1 << 18)


class options:
    """Library options set for a block and restored after it."""

    def __init__(self, wc, ctx, pairs):
        self.ctx = ctx
        self.pairs = [(getattr(wc.capi, k) if isinstance(k, str) else k, v) for k, v in pairs]

    def __enter__(self):
        self.before = [(k, self.ctx.get_option(k)) for k, _ in self.pairs]
        for k, v in self.pairs:
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.before:
            self.ctx.set_option(k, v)


def rmse_agrees(got, ref, ncells):
    if np.isnan(ref):
        return bool(np.isnan(got))
    if np.isinf(ref):
        return got == ref
    return abs(got - ref) <= max(1e-12, (ncells + 4) * 2.0 ** -53) * abs(ref)


# ---- the multi-level transform ------------------------------------------------------------------

class LevelsCase(Batch):
    """A levels batch with its reference results (test_gpu_levels.Batch computes each
    once and leaves it unchanged), the synthesis of the reference's flat arrays
    and the explicit threshold of the batch."""

    def __init__(self, wc, oracle, LB):
        boxes = [b if LB.dtype == np.float64 else b.astype(np.float32) for b in LB.boxes]
        super().__init__(wc, oracle, (LB.dims, LB.levels, boxes, LB.offsets), LB.dtype)
        assert self.extent == LB.extent
        self.keep, self.tags = LB.keep, LB.tags
        self.owned = np.zeros(max(self.extent, 1), bool)
        for i, b in enumerate(self.boxes):
            o = self.units[i].cell_offset
            self.owned[o:o + b.size] = True
        self._synth = {}
        # an explicit threshold that neither keeps everything nor nothing: the 0.7 quantile of
        # the batch's finite non-zero |final coefficients|
        mags = np.abs(np.concatenate([self.flat(i) for i in range(self.n)]).astype(np.float64))
        mags = mags[np.isfinite(mags) & (mags > 0)]
        self.thresh = float(np.float32(np.quantile(mags, 0.7)))
        assert 0.0 < self.thresh < np.inf

    def synth(self, i):
        if i not in self._synth:
            (W, H, D), b = self.dims[i], self.boxes[i]
            self._synth[i] = R.inverse(self.flat(i), W, H, D, self.levels[i]) if b.size else b
        return self._synth[i]


_levels_cases = {}


def levels_case(wc, oracle, seed):
    if seed not in _levels_cases:
        _levels_cases[seed] = LevelsCase(wc, oracle, M.levels_batch(oracle, seed))
    return _levels_cases[seed]


def check_floats(B, buf, want, what):
    """buf: a float output of B.extent elements; want(i): unit i's reference array."""
    assert buf.size == B.owned.size
    for i in range(B.n):
        o, b = B.units[i].cell_offset, B.boxes[i]
        assert same_cells(buf[o:o + b.size], np.asarray(want(i)).ravel()), (what, i, B.dims[i], B.levels[i])
    assert np.all(buf[~B.owned] == SENTINEL), (what, "written outside the units")


def check_payloads(B, payloads, kept, off, keep, thresh, what):
    slot = 4
    for i in range(B.n):
        want, k = B.payload(i, keep, thresh)
        at = (what, i, B.dims[i], B.levels[i], keep, thresh)
        assert int(kept[i]) == k, at
        assert payloads[i] == want, at
        if off is not None:
            assert int(off[i]) == slot, at  # the slot rule of wc_forward: unchanged
            slot += 24 + 8 * B.boxes[i].size
    if off is not None:
        assert int(off[B.n]) == int(off[B.n - 1]) + 20 + 8 * int(kept[B.n - 1]), what


def run_levels_device(wc, ctx, B, what):
    import torch
    d = Dev(wc, B)
    ctx.decompose_levels(d.cells.data_ptr(), d.code, B.units, B.n, B.levels, d.flat.data_ptr())
    ctx.synchronize()
    check_floats(B, d.flat.cpu().numpy(), B.flat, (what, "decompose"))
    ref_flat = np.full(max(B.extent, 1), -5.0, np.float32)  # the reference's flat arrays through the synthesis alone
    for i in range(B.n):
        o = B.units[i].cell_offset
        ref_flat[o:o + B.boxes[i].size] = B.flat(i)
    d.flat.copy_(torch.from_numpy(ref_flat))
    torch.cuda.synchronize()
    ctx.inverse_flat_levels(d.flat.data_ptr(), B.units, B.n, B.levels, d.out.data_ptr())
    ctx.synchronize()
    check_floats(B, d.out.cpu().numpy(), B.synth, (what, "inverse_flat"))
    for keep, thresh in ((B.keep, None), (None, B.thresh)):
        d.pay.fill_(0xA5), d.off.fill_(-3), d.kept.fill_(-1), d.out.fill_(SENTINEL)
        torch.cuda.synchronize()
        ctx.forward_levels(d.cells.data_ptr(), d.code, B.units, B.n, B.levels, keep if keep is not None else 0.5,
                           thresh, *d.out_args())
        ctx.synchronize()
        check_payloads(B, *d.read(), keep, thresh, (what, "forward"))
        ctx.inverse_levels(d.pay.data_ptr(), d.off.data_ptr(), B.units, B.n, B.levels, d.out.data_ptr())
        ctx.synchronize()
        check_floats(B, d.out.cpu().numpy(), lambda i: B.regen(i, keep, thresh), (what, "inverse", keep, thresh))


def run_levels_host(wc, ctx, B, chunk):
    with options(wc, ctx, [(WC_OPT_HOST_CHUNK, chunk)]):
        for keep, thresh in ((B.keep, None), (None, B.thresh)):
            payload, offs, kept = ctx.forward_levels_host(B.cells, B.units, B.n, B.levels,
                                                          keep if keep is not None else 0.5, thresh)
            pos = 4
            for i in range(B.n):
                assert int(offs[i]) == pos, (chunk, i)  # packed as wc_forward_host
                pos += 24 + 8 * int(kept[i])
            check_payloads(B, [wc.capi.unit_payload(payload, offs, kept, i) for i in range(B.n)], kept, None, keep,
                           thresh, ("forward host", chunk))
            for lv in (B.levels, None):  # given, or read from the headers
                out = np.full(max(B.extent, 1), SENTINEL, np.float32)
                ctx.inverse_levels_host(payload, offs[:B.n], B.units, B.n, B.extent, levels=lv, out=out)
                check_floats(B, out, lambda i: B.regen(i, keep, thresh), ("inverse host", chunk, lv is None))


@pytest.mark.parametrize("seed", range(_N or 4))
def test_levels_random_batches(wc, ctx, oracle, seed):
    """wc_decompose_levels, wc_inverse_flat_levels, wc_forward_levels under the
    batch's float32 keep and under one explicit threshold, wc_inverse_levels and
    the _host forms (levels given and NULL; WC_OPT_HOST_CHUNK one run, 2^14 or
    2^18 cells) on modes_batches.levels_batch(seed)."""
    B = levels_case(wc, oracle, seed)
    run_levels_device(wc, ctx, B, seed)
    run_levels_host(wc, ctx, B, int(np.random.default_rng(seed).choice(HOST_CHUNKS)))


@pytest.mark.parametrize("opts", LOOKBACK)
def test_levels_option_paths(wc, ctx, oracle, opts):
    """The device calls of test_levels_random_batches on one batch under the
    ticket look-back, the reversed tile order, a wait bound of one poll and
    both of those: the same bytes and cells, the options restored afterwards."""
    B = levels_case(wc, oracle, 0)
    with options(wc, ctx, _OPTION_SETS[opts]):
        run_levels_device(wc, ctx, B, opts)


# (tag, L) -> kept at keep 0, float32(0.999), 1.0 and 1.5 on a 16^3 box: what the keep rule
# (signed value at the first largest |c|, times 1 - keep; |c| > thresh kept; NaN never) gives.
# nan_first, and every case whose NaN the pyramid carries to A[0] at L = 4: a NaN threshold.
# A +inf first: thresh +inf (nothing), NaN at keep 1, -inf at 1.5 (every non-NaN coefficient:
# 4 of the 4096 are NaN for inf_pair, 11 for inf_block).  A -inf first: the mirror image.
# neg_const: thresh -3 (1 - keep) keeps all until it reaches -0 (the non-zero ones: the 4^3 or
# the single low-pass coefficient) and +1.5.
KEY_CASES = {
    ("nan_first", 2): (0, 0, 0, 0), ("nan_first", 4): (0, 0, 0, 0),
    ("inf_pair", 2): (0, 0, 0, 4092), ("inf_pair", 4): (0, 0, 0, 0),
    ("inf_block", 2): (0, 0, 0, 4085), ("inf_block", 4): (0, 0, 0, 0),
    ("plus_inf", 2): (0, 0, 0, 4096), ("plus_inf", 4): (0, 0, 0, 4096),
    ("minus_inf", 2): (4096, 4096, 0, 0), ("minus_inf", 4): (4096, 4096, 0, 0),
    ("neg_const", 2): (4096, 4096, 64, 64), ("neg_const", 4): (4096, 4096, 1, 1),
}
KEY_KEEPS = (0.0, float(np.float32(0.999)), 1.0, 1.5)


def test_levels_key_cases(wc, ctx, oracle):
    """The keep rule on the FINAL array (k_level_key, a second implementation of
    the key pass) where it is decided by a special: each case at L = 2 and at
    16^3's largest L = 4, the kept counts as literals so that no case can turn
    into an ordinary one, then the payloads and cells as everywhere."""
    import torch
    spec = list(KEY_CASES)
    dims = [(16, 16, 16)] * len(spec)
    boxes = [M.special_box(tag, d, np.random.default_rng(9000)).astype(np.float32) for (tag, _), d in zip(spec, dims)]
    B = Batch(wc, oracle, (dims, [L for _, L in spec], boxes, None), np.float32)
    B.owned = np.ones(B.extent, bool)
    assert R.levels_for(16, 16, 16, 4) == 4
    d = Dev(wc, B)
    for keep, col in zip(KEY_KEEPS, range(4)):
        for i, key in enumerate(spec):
            assert B.payload(i, keep)[1] == KEY_CASES[key][col], (key, keep)
        d.pay.fill_(0xA5), d.off.fill_(-3), d.kept.fill_(-1), d.out.fill_(SENTINEL)
        torch.cuda.synchronize()
        ctx.forward_levels(d.cells.data_ptr(), d.code, B.units, B.n, B.levels, keep, None, *d.out_args())
        ctx.synchronize()
        payloads, kept, off = d.read()
        assert [int(k) for k in kept] == [KEY_CASES[key][col] for key in spec], keep
        check_payloads(B, payloads, kept, off, keep, None, "key cases")
        ctx.inverse_levels(d.pay.data_ptr(), d.off.data_ptr(), B.units, B.n, B.levels, d.out.data_ptr())
        ctx.synchronize()
        check_floats(B, d.out.cpu().numpy(), lambda i: B.regen(i, keep), ("key cases inverse", keep))
    # the synthesis met inf - inf: cells that are NaN where no kept coefficient was
    i = spec.index(("inf_pair", 2))
    assert np.isnan(B.regen(i, 1.5)).any() and not np.isnan(B.boxes[i]).any()


# ---- the reduced-resolution decode --------------------------------------------------------------

def check_coarse(case, cells, what):
    assert cells.size == case.extent
    for i, (w, h, d) in enumerate(case.cdims):
        o = case.out_units[i].cell_offset
        assert same_cells(cells[o:o + w * h * d], case.want[i].ravel()), \
            (what, i, case.dims[i], case.levels[i], case.reduce[i])
    assert np.all(cells[~case.owned()] == SENTINEL), (what, "written outside the units")


@pytest.mark.parametrize("seed", range(_N or 3))
def test_coarse_random_batches(wc, ctx, oracle, seed):
    """wc_inverse_coarse with the levels given and wc_inverse_coarse_host with
    them given and NULL (WC_OPT_HOST_CHUNK as above) on
    modes_batches.coarse_cases of the levels batch; on the first seed once more
    per look-back option set."""
    pays, reduce, odd_at, _ = M.coarse_cases(oracle, M.levels_batch(oracle, seed), np.random.default_rng(7500 + seed))
    case = Case(wc, pays, reduce, odd_at=odd_at)
    assert case.out_units[odd_at].cell_offset % 2 == 1
    check_coarse(case, run_device(ctx, case), (seed, "device"))
    chunk = int(np.random.default_rng(seed).choice(HOST_CHUNKS))
    with options(wc, ctx, [(WC_OPT_HOST_CHUNK, chunk)]):
        for lv in (case.levels, None):
            check_coarse(case, run_host(ctx, case, lv), (seed, "host", chunk, lv is None))
    if seed == 0:
        for opts in LOOKBACK:
            with options(wc, ctx, _OPTION_SETS[opts]):
                check_coarse(case, run_device(ctx, case), (seed, opts))


# ---- the RMSE-tolerance mode --------------------------------------------------------------------

class TolCase:
    """A tolerance batch with the rule's results on the oracle's coefficients, each
    (unit, tolerance) computed once: (thresh, bound, payload bytes, kept)."""

    def __init__(self, wc, oracle, TB):
        self.O, self.dims, self.n, self.dtype = oracle, TB.dims, TB.n, TB.dtype
        self.units, n, self.extent = wc.capi.make_units(TB.dims, offsets=TB.offsets)
        assert n == TB.n and self.extent == TB.extent
        self.cells = np.zeros(max(self.extent, 1), TB.dtype)
        self.boxes = []
        for o, b in zip(TB.offsets, TB.boxes):
            self.cells[o:o + b.size] = b.ravel().astype(TB.dtype)
            self.boxes.append(M.narrow(oracle, b, TB.dtype))
        self.tol = list(TB.tol)
        perm = np.random.default_rng(8500 + TB.seed).permutation(self.n)
        self.tol2 = [self.tol[j] for j in perm]
        self._hist, self._want = {}, {}

    def want(self, i, tol):
        if (i, tol) not in self._want:
            b = self.boxes[i]
            if i not in self._hist:
                with np.errstate(all="ignore"):
                    self._hist[i] = self.O.magnitude_hist(self.O.wavelet_decompose(b))
            t, bd = tol_rule(self._hist[i], b.size, tol)
            p = self.O.compress_payload_thresh(b, t)
            self._want[(i, tol)] = (t, bd, p, int(np.frombuffer(p[16:20], "<i4")[0]))
        return self._want[(i, tol)]


_tol_cases = {}


def tol_case(wc, oracle, seed):
    if seed not in _tol_cases:
        _tol_cases[seed] = TolCase(wc, oracle, M.tol_batch(oracle, seed))
    return _tol_cases[seed]


def check_tol(T, out, tols, what):
    payloads, kept, off, thresh, bound = out
    slot = 4
    for i in range(T.n):
        t, bd, p, k = T.want(i, tols[i])
        at = (what, i, T.dims[i], tols[i])
        assert same_bits(float(thresh[i]), t, np.float32), (at, float(thresh[i]), t)
        assert same_bits(float(bound[i]), bd), (at, float(bound[i]), bd)
        assert int(kept[i]) == k, at
        assert payloads[i] == p, at
        assert int(off[i]) == slot, at  # the slot rule of wc_forward
        slot += 24 + 8 * T.boxes[i].size
    assert int(off[T.n]) == int(off[T.n - 1]) + 20 + 8 * int(kept[T.n - 1]), what


def run_tol_device(wc, ctx, T, what):
    import torch
    d = TolDev(wc, T.cells, T.units, T.n)
    ctx.forward_tol(d.cells.data_ptr(), d.dtype, T.units, T.n, T.tol, *d.out_args())
    ctx.synchronize()
    check_tol(T, d.read(), T.tol, (what, "forward_tol"))
    d = TolDev(wc, T.cells, T.units, T.n)
    ctx.forward_stage(d.cells.data_ptr(), d.dtype, T.units, T.n, None)
    for tols in (T.tol, T.tol2):  # the staged coefficients serve both emits
        d.kept.fill_(-1), d.thresh.fill_(-7.0), d.bound.fill_(-7.0)
        torch.cuda.synchronize()
        ctx.forward_emit_tol(T.units, T.n, tols, *d.out_args())
        ctx.synchronize()
        check_tol(T, d.read(), tols, (what, "stage + emit_tol", tols is T.tol2))


@pytest.mark.parametrize("solo_tiles", [64, 1])
@pytest.mark.parametrize("seed", range(_N or 3))
def test_tol_random_batches(wc, ctx, oracle, seed, solo_tiles):
    """wc_forward_tol, wc_forward_stage + wc_forward_emit_tol twice (the second
    with the tolerances permuted) and wc_forward_tol_host on
    modes_batches.tol_batch(seed), binned by one workgroup per unit
    (WC_OPT_TOL_SOLO_TILES = 64) and split (1); the look-back option sets once."""
    T = tol_case(wc, oracle, seed)
    with options(wc, ctx, [(WC_OPT_TOL_SOLO_TILES, solo_tiles)]):
        run_tol_device(wc, ctx, T, (seed, solo_tiles))
        payload, offs, kept, thresh, bound, rmse = ctx.forward_tol_host(T.cells, T.units, T.n, T.tol)
        pos = 4
        for i in range(T.n):
            t, bd, p, k = T.want(i, T.tol[i])
            at = (seed, solo_tiles, "host", i, T.dims[i], T.tol[i])
            assert int(offs[i]) == pos and int(kept[i]) == k, at  # packed as wc_forward_host
            pos += 24 + 8 * k
            assert wc.capi.unit_payload(payload, offs, kept, i) == p, at
            assert same_bits(float(thresh[i]), t, np.float32) and same_bits(float(bound[i]), bd), at
            with np.errstate(all="ignore"):
                ref = oracle.rmse(T.boxes[i], oracle.decompress_payload(p))
            assert rmse_agrees(rmse[i], ref, T.boxes[i].size), (at, rmse[i], ref)
        if seed == 0 and solo_tiles == 64:
            for opts in LOOKBACK:
                with options(wc, ctx, _OPTION_SETS[opts]):
                    run_tol_device(wc, ctx, T, (seed, opts))


# ---- wc_forward_stage's ADD into d_hist ---------------------------------------------------------

def test_histogram_accumulates(wc, ctx, oracle):
    """wc_forward_stage ADDS the batch's bins to d_hist (include/wavelet_amd.h):
    two batches into the same bins without zeroing between them give the sum;
    bins prefilled just below 2^32 and above 2^40 give prefill + batch (the carry
    into the high word); with d_hist = NULL, stage + emit (thresh = NULL) gives
    wc_forward's bytes.  The batches: two small draws of test_gpu_fuzz._batch."""
    import torch
    dev = torch.device("cuda", 0)
    batches = []
    for seed in (314, 389):
        boxes, dims, offs, extent, dtype, keep = _batch(oracle, seed)
        assert extent < 1 << 19  # small
        fast = [w * h * d > 0 and w % 2 == 0 and h % 2 == 0 and d % 8 == 0 for w, h, d in dims]
        assert any(fast) and not all(fast)  # K1 bins the fast units as it stages them, k_hist the generic ones
        units, n, _ = wc.capi.make_units(dims, offsets=offs)
        host = np.zeros(max(extent, 1), dtype)
        for o, b in zip(offs, boxes):
            host[o:o + b.size] = b.ravel().astype(dtype)
        with np.errstate(all="ignore"):
            want = sum(oracle.magnitude_hist(oracle.wavelet_decompose(M.narrow(oracle, b, dtype))) for b in boxes)
        code = wc.capi.WC_F64 if dtype == np.float64 else wc.capi.WC_F32
        batches.append((torch.from_numpy(host).to(dev), code, units, n, keep, want.astype(np.uint64)))
    (cells_a, code_a, units_a, n_a, keep_a, want_a), (cells_b, code_b, units_b, n_b, _, want_b) = batches
    assert np.any(want_a >= 3) and np.any(want_a == 0) and np.any((want_a > 0) & (want_b > 0))

    def bins(prefill):
        h = torch.from_numpy(prefill.view(np.int64).copy()).to(dev)
        torch.cuda.synchronize()
        return h

    def read(h):
        return h.cpu().numpy().view(np.uint64)

    h = bins(np.zeros(wc.capi.HIST_BINS, np.uint64))
    ctx.forward_stage(cells_a.data_ptr(), code_a, units_a, n_a, h.data_ptr())
    ctx.synchronize()
    assert np.array_equal(read(h), want_a)
    ctx.forward_stage(cells_b.data_ptr(), code_b, units_b, n_b, h.data_ptr())  # not zeroed: A + B
    ctx.synchronize()
    assert np.array_equal(read(h), want_a + want_b)
    prefill = np.where(want_a > 0, np.uint64(2 ** 32 - 3), np.uint64(2 ** 40 + 1))
    h = bins(prefill)
    ctx.forward_stage(cells_a.data_ptr(), code_a, units_a, n_a, h.data_ptr())
    ctx.synchronize()
    assert np.array_equal(read(h), prefill + want_a)
    assert np.any((prefill + want_a) >> np.uint64(32) != prefill >> np.uint64(32))  # a carry happened

    cap = wc.capi.payload_bound(units_a, n_a)

    def outs():
        o = (torch.full((cap,), 0xA5, dtype=torch.uint8, device=dev),
             torch.full((n_a + 1,), -3, dtype=torch.int64, device=dev),
             torch.full((n_a,), -1, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        return o

    def unpack(o):
        pay, off, kept = o[0].cpu().numpy(), o[1].cpu().numpy().view(np.uint64), o[2].cpu().numpy().view(np.uint32)
        return [wc.capi.unit_payload(pay, off, kept, i) for i in range(n_a)], off.tobytes(), kept.tobytes()

    direct, staged = outs(), outs()
    ctx.forward(cells_a.data_ptr(), code_a, units_a, n_a, keep_a, direct[0].data_ptr(), cap, direct[1].data_ptr(),
                direct[2].data_ptr())
    ctx.forward_stage(cells_a.data_ptr(), code_a, units_a, n_a, None)
    ctx.forward_emit(units_a, n_a, keep_a, None, staged[0].data_ptr(), cap, staged[1].data_ptr(),
                     staged[2].data_ptr())
    ctx.synchronize()
    assert unpack(staged) == unpack(direct)
