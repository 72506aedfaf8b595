"""GPU: progressive layers in the compressed domain (include/wavelet_amd.h
wc_split_budget / wc_split_thresh / wc_merge and their _host forms) against the
numpy restatement of the rule (layers_rule.py).  Every comparison is byte equality.

Split: the mixed batch of test_gpu_thin (pair counts 0..8193 around the wave and the
4096-pair tile, a dropped middle tile, first and last pair dropped, K = 0, K >=
pairs, ties, L = 1..4, box (0, 4, 4), overshoot and surplus units) under every
look-back option set and both select paths.  Both outputs are byte-exact, the base
buffer equals wc_thin_budget's / wc_thin_thresh's whole buffer, sentinel included;
counts, T, thresholds and offsets are checked; no byte outside a unit's 20 + 8
pairs is written in either buffer.

Merge: one batch of (a, b) pairs over boxes (32, 16, 32), (33, 17, 31), 16^3 and
(0, 4, 4) (_merge_units() below lists what it holds), under the same option sets;
merge(a, b) == merge(b, a); overlaps, a levels mismatch and a packed unit among
good units.

Then the device identity wc_merge(wc_split_*(P)) == P on wc_forward_levels(thresh =
0) payloads with wc_inverse_levels of both bit-equal, refused calls, the host forms
over several WC_OPT_HOST_CHUNK runs, and one chained call sequence without a sync on
a caller's stream.  The references are computed once and left unchanged."""
import numpy as np
import pytest

import layers_rule as LR
import pack_rule as PR
import thin_rule as TR
from test_gpu_fuzz import _OPTION_SETS
from test_gpu_modes_fuzz import LOOKBACK, options
from test_gpu_thin import BOX4, BOX5, SENT_K, SENT_T, TILE, Dev as ThinDev, _values, mixed
from tol_rule import field, same_bits
from wavelet_compression_amd.capi import WC_MAX_LEVELS, WC_OPT_HOST_CHUNK, WC_OPT_TOL_SOLO_TILES

pytestmark = pytest.mark.gpu

CUBE = (16, 16, 16)
COUNTS = (1, 63, 64, 65, 4095, 4096, 4097, 8193)
_memo = {}


def _opts(opts, solo=None):
    return (() if opts == "default" else _OPTION_SETS[opts]) + (() if solo is None else ((WC_OPT_TOL_SOLO_TILES, solo),))


# ---- split ---------------------------------------------------------------------------------------------------
def split_want(wc):
    """Per unit of the mixed batch: layers_rule's (base, rest, kept, rest pairs, T, thresholds), budget and threshold form."""
    if "split" not in _memo:
        C = mixed(wc)
        wb = [LR.split_budget(u.payload, K) for u, K in zip(C.us, C.K)]
        wt = [LR.split_thresh(u.payload, C.thresh[i, :u.L]) for i, u in enumerate(C.us)]
        for i, u in enumerate(C.us):  # the base is the thinning's; the two forms agree at the thresholds of T
            assert wb[i][0] == C.want[i][0] == wt[i][0] and wb[i][1] == wt[i][1], u.name
            assert LR.merge(wb[i][0], wb[i][1]) == LR.canon(u.payload), u.name
        _memo["split"] = (wb, wt)
    return _memo["split"]


class SplitDev:
    """Device buffers of one split call, prefilled with sentinels."""

    def __init__(self, wc, C, budget, buf=None):
        import torch
        dev = torch.device("cuda", 0)
        self.C, self.budget = C, budget
        self.pay = torch.from_numpy(C.buf if buf is None else buf).to(dev)
        self.off = torch.from_numpy(C.off.view(np.int64)).to(dev)
        self.bslot, self.bext = C.slots(budget)
        self.rslot, self.rext = C.slots(False)
        assert (self.bext, self.rext) == wc.capi.split_bound(C.units, C.n, C.K if budget else None)
        assert self.rext == wc.capi.payload_bound(C.units, C.n)
        self.base = torch.full((self.bext + 32,), 0xA5, dtype=torch.uint8, device=dev)
        self.rest = torch.full((self.rext + 32,), 0xA5, dtype=torch.uint8, device=dev)
        self.boff = torch.full((C.n + 1,), -3, dtype=torch.int64, device=dev)
        self.roff = torch.full((C.n + 1,), -3, dtype=torch.int64, device=dev)
        self.kept = torch.full((C.n,), -1, dtype=torch.int32, device=dev)
        self.rpairs = torch.full((C.n,), -1, dtype=torch.int32, device=dev)
        self.thresh = torch.full((C.n, WC_MAX_LEVELS), SENT_T, dtype=torch.float32, device=dev)
        self.key = torch.full((C.n,), SENT_K, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()  # the fills run on torch's stream, the context on its own

    def run(self, ctx, units=None, levels=None, bcap=None, rcap=None, pay=None, base=None, rest=None):
        C = self.C
        a = (self.pay.data_ptr() if pay is None else pay, self.off.data_ptr(), C.units if units is None else units, C.n,
             C.levels if levels is None else levels)
        b = (self.base.data_ptr() if base is None else base, self.bext if bcap is None else bcap, self.boff.data_ptr(),
             self.kept.data_ptr(), self.rest.data_ptr() if rest is None else rest, self.rext if rcap is None else rcap,
             self.roff.data_ptr(), self.rpairs.data_ptr())
        if self.budget:
            ctx.split_budget(*a, C.K, *b, self.thresh.data_ptr(), self.key.data_ptr())
        else:
            ctx.split_thresh(*a, C.thresh, *b)

    def untouched(self):
        return (all(bool((t == 0xA5).all()) for t in (self.base, self.rest)) and
                all(bool((t == -3).all()) for t in (self.boff, self.roff)) and
                all(bool((t == -1).all()) for t in (self.kept, self.rpairs)) and
                bool((self.thresh == SENT_T).all()) and bool((self.key == SENT_K).all()) and
                self.pay.cpu().numpy().tobytes() == self.C.buf.tobytes())

    def check(self, want, what, skip=()):
        C = self.C
        base, rest = self.base.cpu().numpy(), self.rest.cpu().numpy()
        boff, roff = self.boff.cpu().numpy().view(np.uint64), self.roff.cpu().numpy().view(np.uint64)
        kept, rpairs = self.kept.cpu().numpy().view(np.uint32), self.rpairs.cpu().numpy().view(np.uint32)
        thresh, key = self.thresh.cpu().numpy(), self.key.cpu().numpy().view(np.uint32)
        eb, er = np.full(base.size, 0xA5, np.uint8), np.full(rest.size, 0xA5, np.uint8)
        for i, u in enumerate(C.us):
            who = (what, i, u.name, u.dims, u.L, C.K[i])
            assert int(boff[i]) == self.bslot[i] and int(roff[i]) == self.rslot[i], who
            if i in skip:
                assert int(kept[i]) == 0 and int(rpairs[i]) == 0, who
                continue
            wb, wr, k, kr = want[i][:4]
            assert (int(kept[i]), int(rpairs[i])) == (k, kr), (who, int(kept[i]), k, int(rpairs[i]), kr)
            eb[self.bslot[i]:self.bslot[i] + len(wb)] = np.frombuffer(wb, np.uint8)
            er[self.rslot[i]:self.rslot[i] + len(wr)] = np.frombuffer(wr, np.uint8)
            assert base[self.bslot[i]:self.bslot[i] + len(wb)].tobytes() == wb, (who, "base")
            assert rest[self.rslot[i]:self.rslot[i] + len(wr)].tobytes() == wr, (who, "rest")
            if self.budget:
                T, th = want[i][4], want[i][5]
                assert int(key[i]) == T, (who, hex(int(key[i])), hex(T))
                for l in range(WC_MAX_LEVELS):
                    w = th[l] if l < u.L else 0.0
                    assert same_bits(float(thresh[i, l]), w, np.float32), (who, l + 1)
        last = C.n - 1
        assert int(boff[C.n]) == self.bslot[last] + 20 + 8 * int(kept[last]), what
        assert int(roff[C.n]) == self.rslot[last] + 20 + 8 * int(rpairs[last]), what
        assert base.tobytes() == eb.tobytes(), (what, "a byte outside the units' base payloads was written")
        assert rest.tobytes() == er.tobytes(), (what, "a byte outside the units' rest payloads was written")
        if not self.budget:
            assert bool((self.thresh == SENT_T).all()) and bool((self.key == SENT_K).all()), what
        assert self.pay.cpu().numpy().tobytes() == C.buf.tobytes(), (what, "the input was written")


@pytest.mark.parametrize("solo", [None, 1])
@pytest.mark.parametrize("opts", ("default",) + LOOKBACK)
def test_split_of_the_mixed_batch_matches_the_restatement(wc, ctx, opts, solo):
    C = mixed(wc)
    wb, wt = split_want(wc)
    with options(wc, ctx, _opts(opts, solo)):
        for budget in (True, False):
            d = SplitDev(wc, C, budget)
            d.run(ctx)
            ctx.synchronize()
            d.check(wb if budget else wt, (opts, solo, "budget" if budget else "thresh"))
            t = ThinDev(wc, C, budget)  # the base is the thinning's buffer, byte for byte
            t.run(ctx)
            ctx.synchronize()
            assert d.base.cpu().numpy().tobytes() == t.out.cpu().numpy().tobytes(), (opts, solo, budget)
            assert d.kept.cpu().numpy().tobytes() == t.kept.cpu().numpy().tobytes()
            assert d.boff.cpu().numpy().tobytes() == t.ooff.cpu().numpy().tobytes()
            assert d.key.cpu().numpy().tobytes() == t.key.cpu().numpy().tobytes()
            assert d.thresh.cpu().numpy().tobytes() == t.thresh.cpu().numpy().tobytes()


def test_split_refusals_leave_the_outputs_untouched(wc, ctx):
    C = mixed(wc)
    INVALID = wc.capi.WC_ERR_INVALID

    def refused(d, **kw):
        with pytest.raises(wc.WaveletError) as ei:
            d.run(ctx, **kw)
        ctx.synchronize()
        assert ei.value.code == INVALID and d.untouched(), kw

    for budget in (True, False):
        d = SplitDev(wc, C, budget)
        refused(d, bcap=d.bext - 1)
        refused(d, rcap=d.rext - 1)
        refused(d, levels=[5] + C.levels[1:])
        refused(d, pay=d.base.data_ptr())  # the input's start inside the base's extent
        refused(d, pay=d.rest.data_ptr())  # ... inside the rest's
        refused(d, rest=d.base.data_ptr() + 16 * (d.bext // 32))  # the rest inside the base


@pytest.mark.parametrize("budget", [True, False])
def test_split_with_a_mismatched_header_and_a_packed_unit_among_good_ones(wc, ctx, budget):
    C = mixed(wc)
    wb, wt = split_want(wc)
    by = {u.name: i for i, u in enumerate(C.us)}
    a, b = by["first-last"], by["K>=pairs"]
    buf = C.buf.copy()
    packed = np.frombuffer(wc.capi.pack_unit(C.us[b].payload, 3), np.uint8)
    o = int(C.off[b])
    buf[o:o + packed.size] = packed
    d = SplitDev(wc, C, budget, buf=buf)
    lv = list(C.levels)
    lv[a] = 1
    dims = list(C.dims)
    dims[a] = (BOX5[0], BOX5[2], BOX5[1])  # the same cell count: the slots do not move
    units, _, _ = wc.capi.make_units(dims)
    d.C = type("Shadow", (), dict(vars(C), buf=buf, units=units, slots=C.slots))()
    d.run(ctx, units=units, levels=lv)
    with pytest.raises(wc.WaveletError) as ei:
        ctx.synchronize()
    assert ei.value.code == wc.capi.WC_ERR_FORMAT
    d.check(wb if budget else wt, ("refused units", budget), skip=(a, b))
    ctx.synchronize()  # the error word is cleared


# ---- merge ---------------------------------------------------------------------------------------------------
class Pair:
    def __init__(self, name, dims, L, pa, pb, rng, past=(0, 0), specials=True):
        """a and b at the positions pa and pb (sorted, below N); past: pairs appended past N on either side."""
        self.name, self.dims, self.L = name, dims, L
        self.N = dims[0] * dims[1] * dims[2]
        self.pay = []
        for pos, extra in ((pa, past[0]), (pb, past[1])):
            pos = np.asarray(pos, np.int64)
            runs = (np.diff(pos, prepend=-1) - 1).astype(np.int64)
            if extra:  # the first of them lands exactly on N, the others behind it
                last = int(pos[-1]) if pos.size else -1
                runs = np.concatenate([runs, [self.N - last - 1], rng.integers(0, 3, extra - 1)])
            bits = _values(rng, runs.size, specials=specials)
            self.pay.append(PR.standard(*dims, L, runs.astype(np.uint32), bits))
        self.live = (len(pa), len(pb))


def _disjoint(rng, N, na, nb):
    pos = rng.choice(N, na + nb, replace=False)
    return np.sort(pos[:na]), np.sort(pos[na:])


def _merge_units():
    rng = np.random.default_rng(9400)
    N4, N5, NC = BOX4[0] * BOX4[1] * BOX4[2], BOX5[0] * BOX5[1] * BOX5[2], 4096
    out = []
    out.append(Pair("alternating", CUBE, 4, np.arange(0, NC, 2), np.arange(1, NC, 2), rng))  # every run across the sources is 0
    out.append(Pair("alternating-4-tiles", BOX4, 2, np.arange(0, N4, 2), np.arange(1, N4, 2), rng))
    out.append(Pair("a-before-b", BOX4, 1, np.arange(100, 5100), np.arange(5100, 11000, 1), rng))
    out.append(Pair("b-before-a", BOX5, 1, np.arange(9000, N5, 2), np.arange(3, 8999, 2), rng))
    out.append(Pair("a-empty", BOX4, 3, [], np.sort(rng.choice(N4, 5000, replace=False)), rng))
    out.append(Pair("b-empty", CUBE, 2, np.sort(rng.choice(NC, 700, replace=False)), [], rng))
    out.append(Pair("both-empty", BOX5, 1, [], [], rng))
    out.append(Pair("no-cells", (0, 4, 4), 1, [], [], rng))
    out.append(Pair("no-cells-L2", (0, 4, 4), 2, [], [], rng))
    pa, pb = _disjoint(rng, N4 - 2, 3000, 3000)
    out.append(Pair("b-at-0-a-at-N-1", BOX4, 1, np.append(pa[pa > 0], N4 - 1), np.insert(pb[pb > 0], 0, 0), rng))
    out.append(Pair("full-box", CUBE, 1, *_disjoint(rng, NC, 1000, NC - 1000), rng))  # pairs(a) + pairs(b) = N
    for i, c in enumerate(COUNTS):  # the counts on either side, the other side small or large
        dims, L = [(BOX4, 1), (BOX5, 1), (BOX4, 3), (BOX4, 2)][i % 4]
        N = dims[0] * dims[1] * dims[2]
        out.append(Pair(f"a={c}/small", dims, L, *_disjoint(rng, N, c, 5), rng))
        out.append(Pair(f"large/b={c}", dims, L, *_disjoint(rng, N, 6000, c), rng))
    out.append(Pair("past-N-in-a", BOX4, 1, *_disjoint(rng, N4, 4000, 4200), rng, past=(300, 0)))
    out.append(Pair("past-N-in-b", BOX5, 1, *_disjoint(rng, N5, 10, 8000), rng, past=(0, 5000)))
    out.append(Pair("past-N-in-both", CUBE, 3, *_disjoint(rng, NC, 2000, 2000), rng, past=(4097, 70)))
    return out


class MergeCase:
    def __init__(self, wc, pairs, seed):
        import decode_payloads as DP
        rng = np.random.default_rng(seed)
        self.ps, self.n = pairs, len(pairs)
        self.dims = [p.dims for p in pairs]
        self.levels = [p.L for p in pairs]
        self.units, _, self.extent = wc.capi.make_units(self.dims)
        self.want = [LR.merge(p.pay[0], p.pay[1]) for p in pairs]
        self.abuf, self.aoff = DP.payload_layout([p.pay[0] for p in pairs], rng)
        self.bbuf, self.boff = DP.payload_layout([p.pay[1] for p in pairs], rng)
        self.slot, o = [], 4
        for p in pairs:
            self.slot.append(o)
            o += 24 + 8 * p.N
        self.cap = o


def merge_case(wc):
    if "merge" not in _memo:
        _memo["merge"] = MergeCase(wc, _merge_units(), 9401)
    return _memo["merge"]


class MergeDev:
    def __init__(self, wc, M, abuf=None, bbuf=None, one_buffer=False):
        import torch
        dev = torch.device("cuda", 0)
        self.M = M
        abuf = M.abuf if abuf is None else abuf
        bbuf = M.bbuf if bbuf is None else bbuf
        if one_buffer:  # a and b in one device buffer, b's offsets shifted
            shift = (abuf.size + 15) // 16 * 16
            both = np.zeros(shift + bbuf.size, np.uint8)
            both[:abuf.size], both[shift:] = abuf, bbuf
            self.a = self.b = torch.from_numpy(both).to(dev)
            boff = M.boff + np.uint64(shift)
        else:
            self.a, self.b = torch.from_numpy(abuf).to(dev), torch.from_numpy(bbuf).to(dev)
            boff = M.boff
        self.inputs = (self.a.cpu().numpy().tobytes(), self.b.cpu().numpy().tobytes())
        self.aoff = torch.from_numpy(M.aoff.view(np.int64)).to(dev)
        self.boff = torch.from_numpy(boff.view(np.int64)).to(dev)
        assert M.cap == wc.capi.merge_bound(M.units, M.n) == wc.capi.payload_bound(M.units, M.n)
        self.out = torch.full((M.cap + 32,), 0xA5, dtype=torch.uint8, device=dev)
        self.ooff = torch.full((M.n + 1,), -3, dtype=torch.int64, device=dev)
        self.pairs = torch.full((M.n,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

    def run(self, ctx, swap=False, units=None, levels=None, cap=None, out=None):
        M = self
        a = (M.a.data_ptr(), M.aoff.data_ptr(), M.b.data_ptr(), M.boff.data_ptr())
        ctx.merge(*(a[2:] + a[:2] if swap else a), self.M.units if units is None else units, self.M.n,
                  self.M.levels if levels is None else levels, self.out.data_ptr() if out is None else out,
                  self.M.cap if cap is None else cap, self.ooff.data_ptr(), self.pairs.data_ptr())

    def untouched(self):
        return (bool((self.out == 0xA5).all()) and bool((self.ooff == -3).all()) and bool((self.pairs == -1).all()) and
                (self.a.cpu().numpy().tobytes(), self.b.cpu().numpy().tobytes()) == self.inputs)

    def check(self, what, skip=(), overlap=()):
        M = self.M
        out = self.out.cpu().numpy()
        ooff, pairs = self.ooff.cpu().numpy().view(np.uint64), self.pairs.cpu().numpy().view(np.uint32)
        expect = np.full(out.size, 0xA5, np.uint8)
        for i, p in enumerate(M.ps):
            who = (what, i, p.name, p.dims, p.L)
            s = M.slot[i]
            assert int(ooff[i]) == s, who
            if i in skip:  # refused by its header: the slot untouched
                assert int(pairs[i]) == 0, who
                continue
            if i in overlap:  # a header with 0 pairs; the bytes past it unspecified, inside the slot
                assert int(pairs[i]) == 0, who
                hdr = np.array([*p.dims, -p.L if p.L >= 2 else p.N, 0], "<i4").tobytes()
                assert out[s:s + 20].tobytes() == hdr, who
                expect[s:s + 20 + 8 * p.N] = out[s:s + 20 + 8 * p.N]
                continue
            w = M.want[i]
            assert int(pairs[i]) == (len(w) - 20) // 8 <= min(p.N, p.live[0] + p.live[1]), (who, int(pairs[i]))
            expect[s:s + len(w)] = np.frombuffer(w, np.uint8)
            assert out[s:s + len(w)].tobytes() == w, who
        assert int(ooff[M.n]) == M.slot[-1] + 20 + 8 * int(pairs[-1]), what
        assert out.tobytes() == expect.tobytes(), (what, "a byte outside the units' payloads was written")
        assert (self.a.cpu().numpy().tobytes(), self.b.cpu().numpy().tobytes()) == self.inputs, (what, "an input was written")


def test_the_merge_batch_shows_what_it_claims(wc):
    M = merge_case(wc)
    by = {p.name: i for i, p in enumerate(M.ps)}
    _, _, _, _, _, runs, _ = TR.parse(M.want[by["alternating"]])
    assert runs.size == 4096 and not runs.any()
    assert {p.dims for p in M.ps} == {BOX4, BOX5, CUBE, (0, 4, 4)} and {p.L for p in M.ps} == {1, 2, 3, 4}
    assert {p.live[0] for p in M.ps} >= set(COUNTS) | {0} and {p.live[1] for p in M.ps} >= set(COUNTS) | {0}
    W, H, D, _, pos, _ = LR.live_pairs(M.want[by["b-at-0-a-at-N-1"]])[:6]
    assert pos[0] == 0 and pos[-1] == W * H * D - 1
    assert LR.live_pairs(M.ps[by["b-at-0-a-at-N-1"]].pay[1])[4][0] == 0
    assert len(M.want[by["full-box"]]) == 20 + 8 * 4096
    for name, side in (("past-N-in-a", 0), ("past-N-in-b", 1), ("past-N-in-both", 0), ("past-N-in-both", 1)):
        p = M.ps[by[name]]
        assert (len(p.pay[side]) - 20) // 8 > p.live[side] == LR.live_pairs(p.pay[side])[4].size, name
    bits = np.concatenate([TR.parse(w)[6] for w in M.want])
    m = bits & 0x7FFFFFFF
    assert (m == 0).any() and (m > 0x7F800000).any() and (m == 0x7F800000).any() and ((m > 0) & (m < 0x00800000)).any()
    assert max(-(-p.live[0] // TILE) for p in M.ps) >= 3


@pytest.mark.parametrize("opts", ("default",) + LOOKBACK)
def test_merge_batch_matches_the_restatement_in_both_orders(wc, ctx, opts):
    M = merge_case(wc)
    with options(wc, ctx, _opts(opts)):
        for swap in (False, True):
            d = MergeDev(wc, M, one_buffer=swap)
            d.run(ctx, swap=swap)
            ctx.synchronize()
            d.check((opts, "b, a" if swap else "a, b"))


def _with_overlaps(M, rng):
    """b's payloads of three large units rebuilt so that one position of a is in b too: a's pair 4096 (a tile's
    first), a's pair 4095 (a tile's last) and a's last live pair.  -> (b buffer, b offsets, their indices)."""
    by = {p.name: i for i, p in enumerate(M.ps)}
    picks = {by["a-before-b"]: 4096, by["alternating-4-tiles"]: 4095, by["large/b=4097"]: -1}
    pays = [p.pay[1] for p in M.ps]
    for i, k in picks.items():
        p = M.ps[i]
        W, H, D, nc, apos, _ = LR.live_pairs(p.pay[0])
        _, _, _, _, bpos, bbits = LR.live_pairs(p.pay[1])
        assert apos.size > 4096 and apos[k] not in bpos
        pos = np.sort(np.append(bpos, apos[k]))
        pays[i] = LR.emit(W, H, D, nc, pos, np.resize(bbits, pos.size))
        with pytest.raises(LR.Overlap):
            LR.merge(p.pay[0], pays[i])
    import decode_payloads as DP
    buf, off = DP.payload_layout(pays, rng)
    return buf, off, tuple(picks)


@pytest.mark.parametrize("opts", ("default", "tickets", "reversed_spin_1"))
def test_merge_overlaps_among_good_units(wc, ctx, opts):
    M = merge_case(wc)
    bbuf, boff, ov = _with_overlaps(M, np.random.default_rng(9402))
    S = type("Shadow", (), dict(vars(M), bbuf=bbuf, boff=boff))()
    with options(wc, ctx, _opts(opts)):
        d = MergeDev(wc, S)
        d.run(ctx)
        with pytest.raises(wc.WaveletError) as ei:
            ctx.synchronize()
        assert ei.value.code == wc.capi.WC_ERR_FORMAT
        d.check(("overlaps", opts), overlap=ov)
        ctx.synchronize()  # the error word is cleared


def test_merge_with_a_levels_mismatch_and_a_packed_unit_among_good_ones(wc, ctx):
    M = merge_case(wc)
    by = {p.name: i for i, p in enumerate(M.ps)}
    x, y = by["alternating-4-tiles"], by["b-empty"]
    pays = [p.pay[1] for p in M.ps]
    other = bytearray(pays[x])  # b's header names L = 3, a's and the call's L = 2
    other[12:16] = np.array([-3], "<i4").tobytes()
    pays[x] = bytes(other)
    apays = [p.pay[0] for p in M.ps]
    packed = wc.capi.pack_unit(apays[y], 3)
    assert len(packed) <= len(apays[y])
    apays[y] = packed + bytes(len(apays[y]) - len(packed))
    import decode_payloads as DP
    rng = np.random.default_rng(9403)
    abuf, aoff = DP.payload_layout(apays, rng)
    bbuf, boff = DP.payload_layout(pays, rng)
    S = type("Shadow", (), dict(vars(M), abuf=abuf, aoff=aoff, bbuf=bbuf, boff=boff))()
    d = MergeDev(wc, S)
    d.run(ctx)
    with pytest.raises(wc.WaveletError) as ei:
        ctx.synchronize()
    assert ei.value.code == wc.capi.WC_ERR_FORMAT
    d.check("refused units", skip=(x, y))
    ctx.synchronize()


def test_merge_refusals_leave_the_outputs_untouched(wc, ctx):
    M = merge_case(wc)
    d = MergeDev(wc, M)
    for kw in (dict(cap=M.cap - 1), dict(levels=[5] + M.levels[1:]), dict(out=d.a.data_ptr()), dict(out=d.b.data_ptr())):
        with pytest.raises(wc.WaveletError) as ei:
            d.run(ctx, **kw)
        ctx.synchronize()
        assert ei.value.code == wc.capi.WC_ERR_INVALID and d.untouched(), kw


# ---- the identity, the decoders, the host forms, the asynchronous contract -----------------------------------
SPEC = [(CUBE, 4, 2), (BOX4, 3, 0), (BOX4, 1, 1), ((8, 8, 8), 2, 0), ((64, 32, 64), 3, 2), (BOX5, 1, 1)]


def _identity_chain(wc, ctx, budget, stream=None):
    """forward(thresh = 0) -> split -> merge -> inverse of the merged and of P, enqueued without a sync.
    -> the device tensors and the expected bytes."""
    import torch
    dims = [s[0] for s in SPEC]
    levels = [s[1] for s in SPEC]
    boxes = [field(k, *d, seed=120 + i).astype(np.float32) for i, (d, _, k) in enumerate(SPEC)]
    units, n, extent = wc.capi.make_units(dims)
    K = [b.size // 5 + i for i, b in enumerate(boxes)]
    th = np.zeros((n, WC_MAX_LEVELS), np.float32)
    th[:] = 0.05
    host = np.zeros(extent, np.float32)
    for i, b in enumerate(boxes):
        host[units[i].cell_offset:units[i].cell_offset + b.size] = b.ravel()
    dev = torch.device("cuda", 0)
    cap = wc.capi.payload_bound(units, n)
    bcap, rcap = wc.capi.split_bound(units, n, K if budget else None)

    def bufs(c):
        return (torch.full((c,), 0xA5, dtype=torch.uint8, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev),
                torch.zeros(n, dtype=torch.int32, device=dev))

    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        cells = torch.from_numpy(host).to(dev)
        full, base, rest, merged = bufs(cap), bufs(bcap), bufs(rcap), bufs(cap)
        back_p = torch.full((extent,), -77.0, dtype=torch.float32, device=dev)
        back_m = torch.full((extent,), -78.0, dtype=torch.float32, device=dev)
        if stream is None:
            torch.cuda.synchronize()
        ctx.forward_levels(cells.data_ptr(), wc.capi.WC_F32, units, n, levels, 0.0, 0.0, full[0].data_ptr(), cap,
                           full[1].data_ptr(), full[2].data_ptr())
        a = (full[0].data_ptr(), full[1].data_ptr(), units, n, levels)
        b = (base[0].data_ptr(), bcap, base[1].data_ptr(), base[2].data_ptr(), rest[0].data_ptr(), rcap, rest[1].data_ptr(),
             rest[2].data_ptr())
        if budget:
            ctx.split_budget(*a, K, *b)
        else:
            ctx.split_thresh(*a, th, *b)
        ctx.merge(rest[0].data_ptr(), rest[1].data_ptr(), base[0].data_ptr(), base[1].data_ptr(), units, n, levels,
                  merged[0].data_ptr(), cap, merged[1].data_ptr(), merged[2].data_ptr())
        ctx.inverse_levels(merged[0].data_ptr(), merged[1].data_ptr(), units, n, levels, back_m.data_ptr())
        ctx.inverse_levels(full[0].data_ptr(), full[1].data_ptr(), units, n, levels, back_p.data_ptr())
    return dict(n=n, units=units, K=K, th=th, full=full, base=base, rest=rest, merged=merged, back_p=back_p, back_m=back_m)


def _check_identity(wc, r, budget):
    def read(b):
        pay, off, kept = b[0].cpu().numpy(), b[1].cpu().numpy().view(np.uint64), b[2].cpu().numpy().view(np.uint32)
        return [wc.capi.unit_payload(pay, off, kept, i) for i in range(r["n"])]

    P, base, rest, merged = read(r["full"]), read(r["base"]), read(r["rest"]), read(r["merged"])
    for i in range(r["n"]):
        assert merged[i] == P[i] and len(P[i]) > 20 + 8 * 100, i
        want = LR.split_budget(P[i], r["K"][i]) if budget else LR.split_thresh(P[i], r["th"][i, :SPEC[i][1]])
        assert (base[i], rest[i]) == want[:2] and 20 < len(base[i]) < len(P[i]), i
    assert r["back_m"].cpu().numpy().tobytes() == r["back_p"].cpu().numpy().tobytes()
    assert not (r["back_p"] == -77.0).any()


@pytest.mark.parametrize("budget", [True, False])
def test_device_identity_merge_of_split_is_the_payload_and_decodes_alike(wc, ctx, budget):
    r = _identity_chain(wc, ctx, budget)
    ctx.synchronize()
    _check_identity(wc, r, budget)


def test_chained_calls_on_a_caller_stream_without_a_sync(wc):
    """forward -> split -> merge -> inverse on a torch stream through wc_set_stream; one wc_synchronize at the end."""
    import torch
    ctx = wc.capi.Context(0)
    s = torch.cuda.Stream()
    try:
        ctx.set_stream(s.cuda_stream)
        r = _identity_chain(wc, ctx, True, stream=s)
        ctx.synchronize()
        _check_identity(wc, r, True)
    finally:
        ctx.set_stream(None)
        ctx.close()


@pytest.mark.parametrize("budget", [True, False])
def test_host_forms_over_several_runs(wc, ctx, budget):
    C = mixed(wc)
    wb, wt = split_want(wc)
    want = wb if budget else wt

    def packed(out, off, cnt, exp, what):
        o = 4  # packed as wc_forward_host: 24 + 8 pairs bytes apart, from 4
        for i, w in enumerate(exp):
            assert int(off[i]) == o and 20 + 8 * int(cnt[i]) == len(w), (what, i)
            assert out[o:o + len(w)].tobytes() == w, (what, i)
            o += len(w) + (4 if i + 1 < len(exp) else 0)
        assert int(off[len(exp)]) == o, what

    with options(wc, ctx, ((WC_OPT_HOST_CHUNK, 1 << 15),)):
        assert sum(u.N for u in C.us) > 2 << 15
        for levels in (None, C.levels):
            base, boff, kept, rest, roff, rpairs, th, key = ctx.split_host(
                C.buf, C.off, C.units, C.n, levels, max_pairs=C.K if budget else None, thresh=None if budget else C.thresh)
            packed(base, boff, kept, [w[0] for w in want], "base")
            packed(rest, roff, rpairs, [w[1] for w in want], "rest")
            for i, u in enumerate(C.us):
                if budget:
                    assert int(key[i]) == want[i][4] and all(
                        same_bits(float(th[i, l]), want[i][5][l] if l < u.L else 0.0, np.float32)
                        for l in range(WC_MAX_LEVELS)), (i, u.name)
            out, off, pairs = ctx.merge_host(rest, roff, base, boff, C.units, C.n, levels)
            packed(out, off, pairs, [LR.canon(u.payload) for u in C.us], "merged")
        M = merge_case(wc)
        assert sum(p.N for p in M.ps) > 4 << 15
        out, off, pairs = ctx.merge_host(M.abuf, M.aoff, M.bbuf, M.boff, M.units, M.n, None)
        packed(out, off, pairs, M.want, "merge batch")
    # a header that disagrees fails the call; so does an overlap, at the call's end
    lv = list(C.levels)
    lv[0] = 2 if lv[0] == 1 else 1
    with pytest.raises(wc.WaveletError) as ei:
        ctx.split_host(C.buf, C.off, C.units, C.n, lv, max_pairs=C.K if budget else None, thresh=None if budget else C.thresh)
    assert ei.value.code == wc.capi.WC_ERR_FORMAT
    with pytest.raises(wc.WaveletError) as ei:
        ctx.merge_host(M.abuf, M.aoff, M.abuf, M.aoff, M.units, M.n, None)  # a with itself
    assert ei.value.code == wc.capi.WC_ERR_FORMAT
