"""GPU: thinning in the compressed domain (include/wavelet_amd.h wc_thin_budget /
wc_thin_thresh and their _host forms) against the numpy restatement of the rule
(thin_rule.py).

Bar: per unit the output bytes, the kept count, T and the per-level thresholds
equal the restatement's bit for bit; the slots follow wc_thin_bound's rule; no
byte of the output buffer outside a unit's 20 + 8 kept bytes is written; a
refused call leaves every output untouched.

One mixed batch (_mixed() below): pair counts around the wave and the pair tile, a
unit of three pair tiles whose whole middle tile a budget drops (the run across
it carries over two tile boundaries), units whose first and whose last pair are
dropped, K = 0, K >= the pair count, a tie at T, boxes 16^3 at L = 4, (32, 16, 32) at
L = 1..3, (33, 17, 31) at L = 1 and (0, 4, 4), the
crafted overshoot and surplus units of decode_payloads, and a unit whose thresholds
are exactly 0.0 over +-0, NaN, +-inf and subnormals.  It runs under every
look-back option set and with both select paths (WC_OPT_TOL_SOLO_TILES 1 and
default).  The references are computed once and left unchanged."""
import numpy as np
import pytest

import budget_rule as BR
import decode_payloads as DP
import levels_ref as R
import pack_rule as PR
import thin_rule as TR
from test_gpu_fuzz import _OPTION_SETS, same_cells
from test_gpu_modes_fuzz import LOOKBACK, options
from tol_rule import field, same_bits
from wavelet_compression_amd.capi import WC_MAX_LEVELS, WC_OPT_HOST_CHUNK, WC_OPT_TOL_SOLO_TILES

pytestmark = pytest.mark.gpu

SENT_T, SENT_K = -7.0, 0x5A5A5A5A
TILE = 4096
BOX4 = (32, 16, 32)   # four pair tiles at most
BOX5 = (33, 17, 31)   # odd, L = 1 only: five
COUNTS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 8193)


def _values(rng, n, specials=True):
    """n value bit patterns: distinct finite magnitudes of either sign, a few +-0, NaN, +-inf, subnormals."""
    mag = rng.permutation(n).astype(np.float64) * 1e-3 + 1.0  # distinct
    v = (mag * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32).view(np.uint32).copy()
    if specials and n >= 16:
        idx = rng.choice(n, 8, replace=False)
        v[idx] = np.array([0, 0x80000000, 0x7FC00000, 0xFF800001, 0x7F800000, 0xFF800000, 1, 0x80000003], np.uint32)
    return v


def _at(rng, N, n):
    """Runs of n pairs at sorted distinct positions below N."""
    pos = np.sort(rng.choice(N, n, replace=False)) if n else np.zeros(0, np.int64)
    return (np.diff(pos, prepend=-1) - 1).astype(np.uint32)


class Unit:
    def __init__(self, name, dims, L, runs, bits, K):
        self.name, self.dims, self.L, self.K = name, dims, L, K
        self.payload = PR.standard(*dims, L, runs, bits)
        self.pairs = len(runs)
        self.N = dims[0] * dims[1] * dims[2]


def _mixed():
    rng = np.random.default_rng(9200)
    N4, N5 = BOX4[0] * BOX4[1] * BOX4[2], BOX5[0] * BOX5[1] * BOX5[2]
    out = []
    for i, n in enumerate(COUNTS):  # the two large boxes and their levels, in turn
        dims, L = [(BOX4, 1), (BOX4, 2), (BOX4, 3), (BOX5, 1)][i % 4]
        out.append(Unit(f"n={n}", dims, L, _at(rng, dims[0] * dims[1] * dims[2], n), _values(rng, n), "rank"))
    # three full pair tiles; the middle one's magnitudes are below all others: K = 2 tiles drops exactly it
    bits = _values(rng, 3 * TILE, specials=False)
    mid = slice(TILE, 2 * TILE)
    bits[mid] = ((bits[mid] & np.uint32(0x7FFFFFFF)).view(np.float32) * np.float32(1e-6)).view(np.uint32)
    out.append(Unit("middle-tile", BOX4, 1, _at(rng, N4, 3 * TILE), bits, 2 * TILE))
    # first and last pair dropped: the two smallest magnitudes
    bits = _values(rng, 5000, specials=False)
    bits[0], bits[-1] = np.float32(1e-3).view(np.uint32), np.float32(-2e-3).view(np.uint32)
    out.append(Unit("first-last", BOX5, 1, _at(rng, N5, 5000), bits, 4998))
    out.append(Unit("K=0", (16, 16, 16), 4, _at(rng, 4096, 700), _values(rng, 700), 0))
    clean = _values(rng, 900, specials=False)
    out.append(Unit("K>=pairs", (16, 16, 16), 4, _at(rng, 4096, 900), clean, 900))
    out.append(Unit("K>pairs", BOX4, 3, _at(rng, N4, 4500), _values(rng, 4500, specials=False), 0xFFFFFFFF))
    # a tie at T: 40 equal magnitudes at one level (L = 1) around the budget
    bits = _values(rng, 6000, specials=False)
    bits[rng.choice(6000, 40, replace=False)] = np.float32(3.25).view(np.uint32)
    out.append(Unit("tie", BOX4, 1, _at(rng, N4, 6000), bits, "tie"))
    out.append(Unit("tie-L3", BOX4, 3, _at(rng, N4, 6000), bits.copy(), "tie"))
    out.append(Unit("L4", (16, 16, 16), 4, _at(rng, 4096, 4096), _values(rng, 4096), "rank"))
    out.append(Unit("empty", (0, 4, 4), 1, np.zeros(0, np.uint32), np.zeros(0, np.uint32), 3))
    out.append(Unit("empty-L2", (0, 4, 4), 2, np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0))
    crafted = [u for u in DP.crafted() if u.dims in (DP.RIX, DP.DENSE[1])]
    over = [u for u in crafted if DP.is_overshoot(u)]
    surplus = [u for u in crafted if DP.is_surplus(u)]
    assert len(over) >= 4 and len(surplus) >= 4
    for u in over[::max(1, len(over) // 4)][:4] + surplus[::max(1, len(surplus) // 4)][:4]:
        out.append(Unit(u.name, u.dims, u.L, u.runs, u.bits, "rank"))
    # thresholds of exactly 0.0 over +-0, NaN, +-inf and subnormals (K above the candidates: T = 0): the one
    # place where "|c| > t" and "a candidate above t" could part.  Last, so the units before it stay as they were.
    out.append(Unit("t=0", (16, 16, 16), 2, _at(rng, 4096, 300), _values(rng, 300), 0xFFFFFFFF))
    return out


class Case:
    """A batch with its restatement results: want[i] = (bytes, kept, T, [thresh_l], ties)."""

    def __init__(self, wc, units, seed):
        rng = np.random.default_rng(seed)
        self.us, self.n = units, len(units)
        self.dims = [u.dims for u in units]
        self.levels = [u.L for u in units]
        self.units, _, self.extent = wc.capi.make_units(self.dims)
        self.K = []
        for u in units:
            if isinstance(u.K, str):
                b = TR.budgets(u.payload, rng)
                assert u.K in b or u.K == "rank", (u.name, u.K, sorted(b))
                self.K.append(b.get(u.K, b["over"]))  # fewer than two candidates: no rank to pick
            else:
                self.K.append(u.K)
        self.want = [TR.thin_budget(u.payload, K) for u, K in zip(units, self.K)]
        self.buf, self.off = DP.payload_layout([u.payload for u in units], rng)
        self.thresh = np.zeros((self.n, WC_MAX_LEVELS), np.float32)
        for i, w in enumerate(self.want):
            self.thresh[i, :len(w[3])] = w[3]
        self.cap = [min(K, u.N) for u, K in zip(units, self.K)]

    def slots(self, budget):
        o, out = 4, []
        for i, u in enumerate(self.us):
            out.append(o)
            o += 24 + 8 * (self.cap[i] if budget else u.N)
        return out, o


_memo = {}


def mixed(wc):
    if "mixed" not in _memo:
        _memo["mixed"] = Case(wc, _mixed(), 9201)
    return _memo["mixed"]


class Dev:
    """Device buffers of one call, prefilled with sentinels."""

    def __init__(self, wc, C, budget, buf=None):
        import torch
        dev = torch.device("cuda", 0)
        self.C, self.budget = C, budget
        self.pay = torch.from_numpy(C.buf if buf is None else buf).to(dev)
        self.off = torch.from_numpy(C.off.view(np.int64)).to(dev)
        self.slot, self.extent = C.slots(budget)
        assert self.extent == wc.capi.thin_bound(C.units, C.n, C.K if budget else None)
        self.out = torch.full((self.extent + 32,), 0xA5, dtype=torch.uint8, device=dev)
        self.ooff = torch.full((C.n + 1,), -3, dtype=torch.int64, device=dev)
        self.kept = torch.full((C.n,), -1, dtype=torch.int32, device=dev)
        self.thresh = torch.full((C.n, WC_MAX_LEVELS), SENT_T, dtype=torch.float32, device=dev)
        self.key = torch.full((C.n,), SENT_K, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()  # the fills run on torch's stream, the context on its own

    def run(self, ctx, units=None, levels=None, K=None, thresh=None, cap=None, nulls=False):
        C = self.C
        a = (self.pay.data_ptr(), self.off.data_ptr(), C.units if units is None else units, C.n,
             C.levels if levels is None else levels)
        b = (self.out.data_ptr(), self.extent if cap is None else cap, self.ooff.data_ptr(), self.kept.data_ptr())
        if self.budget:
            ctx.thin_budget(*a, C.K if K is None else K, *b, *(() if nulls else (self.thresh.data_ptr(), self.key.data_ptr())))
        else:
            ctx.thin_thresh(*a, C.thresh if thresh is None else thresh, *b)

    def untouched(self):
        return (bool((self.out == 0xA5).all()) and bool((self.ooff == -3).all()) and bool((self.kept == -1).all())
                and bool((self.thresh == SENT_T).all()) and bool((self.key == SENT_K).all())
                and self.pay.cpu().numpy().tobytes() == self.C.buf.tobytes())

    def check(self, what, skip=(), selection=True):
        C = self.C
        out = self.out.cpu().numpy()
        ooff = self.ooff.cpu().numpy().view(np.uint64)
        kept = self.kept.cpu().numpy().view(np.uint32)
        thresh, key = self.thresh.cpu().numpy(), self.key.cpu().numpy().view(np.uint32)
        expect = np.full(out.size, 0xA5, np.uint8)
        for i, u in enumerate(C.us):
            who = (what, i, u.name, u.dims, u.L, C.K[i])
            assert int(ooff[i]) == self.slot[i], who
            if i in skip:
                assert int(kept[i]) == 0, who
                continue
            pay, k, T, th, _ = C.want[i]
            assert int(kept[i]) == k and k <= min(C.K[i], u.pairs), (who, int(kept[i]), k)
            assert len(pay) <= len(u.payload), who
            expect[self.slot[i]:self.slot[i] + len(pay)] = np.frombuffer(pay, np.uint8)
            got = out[self.slot[i]:self.slot[i] + len(pay)].tobytes()
            assert got == pay, who
            if self.budget and selection:
                assert int(key[i]) == T, (who, hex(int(key[i])), hex(T))
                for l in range(WC_MAX_LEVELS):
                    w = th[l] if l < u.L else 0.0
                    assert same_bits(float(thresh[i, l]), w, np.float32), (who, l + 1, float(thresh[i, l]), w)
        last = C.n - 1
        assert int(ooff[C.n]) == self.slot[last] + 20 + 8 * int(kept[last]), what
        assert out.tobytes() == expect.tobytes(), (what, "a byte outside the units' payloads was written")
        if not self.budget or not selection:
            assert bool((self.thresh == SENT_T).all()) and bool((self.key == SENT_K).all()), what
        assert self.pay.cpu().numpy().tobytes() == C.buf.tobytes(), (what, "the input was written")


def test_the_batch_shows_what_it_claims(wc):
    C = mixed(wc)
    by = {u.name: i for i, u in enumerate(C.us)}
    assert sorted(u.pairs for u in C.us[:len(COUNTS)]) == sorted(COUNTS)
    i = by["middle-tile"]
    W, H, D, L, _, runs, bits = TR.parse(C.us[i].payload)
    _, _, _, _, _, oruns, obits = TR.parse(C.want[i][0])
    assert C.want[i][1] == 2 * TILE and C.want[i][4] == 1
    assert np.array_equal(obits, np.concatenate([bits[:TILE], bits[2 * TILE:]]))  # exactly the middle tile is gone
    assert int(oruns[TILE]) >= TILE  # the run across it
    i = by["first-last"]
    _, _, _, _, _, _, bits = TR.parse(C.us[i].payload)
    _, _, _, _, _, _, obits = TR.parse(C.want[i][0])
    assert np.array_equal(obits, bits[1:-1])
    assert C.want[by["K=0"]][0][16:20] == b"\0\0\0\0" and len(C.want[by["K=0"]][0]) == 20
    assert C.want[by["K>=pairs"]][0] == C.us[by["K>=pairs"]].payload
    assert C.want[by["K>pairs"]][0] == C.us[by["K>pairs"]].payload
    for name in ("tie", "tie-L3"):
        assert C.want[by[name]][4] >= 2 and C.want[by[name]][1] < C.K[by[name]]
    i = by["t=0"]
    _, _, _, _, _, _, bits = TR.parse(C.us[i].payload)
    m = bits & np.uint32(0x7FFFFFFF)
    assert C.want[i][2] == 0 and not C.thresh[i].any()  # T = 0: the threshold form runs it at 0.0 on both levels
    assert {0, 0x80000000, 0x7F800000, 0xFF800000} <= set(bits.tolist())
    assert ((m > 0) & (m < 0x00800000)).any() and (m > 0x7F800000).any()  # a subnormal, a NaN
    assert C.want[i][1] == int(((m >= 1) & (m <= 0x7F800000)).sum()) < C.us[i].pairs  # every candidate, no other pair
    assert {u.dims for u in C.us} >= {(16, 16, 16), BOX4, BOX5, (0, 4, 4)}
    assert {(u.dims, u.L) for u in C.us} >= {((16, 16, 16), 4), (BOX4, 1), (BOX4, 2), (BOX4, 3), (BOX5, 1)}
    tiles = [-(-min(u.pairs, u.N) // TILE) for u in C.us]
    assert max(tiles) >= 3 and min(tiles) == 0


@pytest.mark.parametrize("solo", [None, 1])
@pytest.mark.parametrize("opts", ("default",) + LOOKBACK)
def test_mixed_batch_matches_the_restatement(wc, ctx, opts, solo):
    C = mixed(wc)
    pairs = (() if opts == "default" else _OPTION_SETS[opts]) + (() if solo is None else ((WC_OPT_TOL_SOLO_TILES, solo),))
    with options(wc, ctx, pairs):
        for budget in (True, False):
            d = Dev(wc, C, budget)
            d.run(ctx)
            ctx.synchronize()
            d.check((opts, solo, "budget" if budget else "thresh"))
    if opts == "default" and solo is None:
        d = Dev(wc, C, True)
        d.run(ctx, nulls=True)  # d_thresh and d_key are nullable
        ctx.synchronize()
        d.check("nulls", selection=False)


def test_host_side_refusals_leave_the_outputs_untouched(wc, ctx):
    C = mixed(wc)
    INVALID = wc.capi.WC_ERR_INVALID

    def refused(d, **kw):
        with pytest.raises(wc.WaveletError) as ei:
            d.run(ctx, **kw)
        ctx.synchronize()
        assert ei.value.code == INVALID and d.untouched(), kw

    for budget in (True, False):
        d = Dev(wc, C, budget)
        refused(d, cap=d.extent - 1)
        refused(d, levels=[5] + C.levels[1:])
        refused(d, levels=[2 if u.dims == BOX5 else u.L for u in C.us])  # 2 does not divide an odd box
    d = Dev(wc, C, False)
    for bad in (np.nan, -1.0):
        t = C.thresh.copy()
        t[3, 0] = bad
        refused(d, thresh=t)
    # the input's start inside the output's extent
    d = Dev(wc, C, True)
    with pytest.raises(wc.WaveletError) as ei:
        ctx.thin_budget(d.out.data_ptr(), d.off.data_ptr(), C.units, C.n, C.levels, C.K, d.out.data_ptr(), d.extent,
                        d.ooff.data_ptr(), d.kept.data_ptr())
    assert ei.value.code == INVALID and d.untouched()


@pytest.mark.parametrize("budget", [True, False])
def test_a_mismatched_header_and_a_packed_unit_among_good_ones(wc, ctx, budget):
    """Unit a is declared with another box, unit b's bytes are a packed unit: WC_ERR_FORMAT at the next
    wc_synchronize, their slots untouched and kept 0, the other units thinned as usual."""
    C = mixed(wc)
    by = {u.name: i for i, u in enumerate(C.us)}
    a, b = by["first-last"], by["K>=pairs"]
    buf = C.buf.copy()
    packed = np.frombuffer(wc.capi.pack_unit(C.us[b].payload, 3), np.uint8)
    assert packed.size <= len(C.us[b].payload)
    o = int(C.off[b])
    buf[o:o + packed.size] = packed
    d = Dev(wc, C, budget, buf=buf)
    lv = list(C.levels)
    lv[a] = 1
    dims = list(C.dims)
    dims[a] = (BOX5[0], BOX5[2], BOX5[1])  # the same cell count: the slots do not move
    units, _, _ = wc.capi.make_units(dims)
    d.C = type("Shadow", (), dict(vars(C), buf=buf, units=units))()
    d.run(ctx, units=units, levels=lv)
    with pytest.raises(wc.WaveletError) as ei:
        ctx.synchronize()
    assert ei.value.code == wc.capi.WC_ERR_FORMAT
    d.check(("refused units", budget), skip=(a, b))
    ctx.synchronize()  # the error word is cleared


@pytest.mark.parametrize("budget", [True, False])
def test_host_forms_in_two_runs(wc, ctx, budget):
    C = mixed(wc)
    with options(wc, ctx, ((WC_OPT_HOST_CHUNK, 1 << 15),)):
        assert sum(u.N for u in C.us) > 2 << 15
        for levels in (None, C.levels):
            out, off, kept, th, key = ctx.thin_host(C.buf, C.off, C.units, C.n, levels,
                                                    max_pairs=C.K if budget else None,
                                                    thresh=None if budget else C.thresh)
            o = 4  # packed as wc_forward_host: 24 + 8 kept bytes apart, from 4
            for i, u in enumerate(C.us):
                pay, k, T, tl, _ = C.want[i]
                assert int(off[i]) == o and int(kept[i]) == k, (i, u.name)
                assert out[o:o + len(pay)].tobytes() == pay, (i, u.name)
                o += 24 + 8 * k if i + 1 < C.n else 20 + 8 * k
                if budget:
                    assert int(key[i]) == T and all(same_bits(float(th[i, l]), tl[l] if l < u.L else 0.0, np.float32)
                                                    for l in range(WC_MAX_LEVELS)), (i, u.name)
            assert int(off[C.n]) == o
    # a header that disagrees fails the call
    lv = list(C.levels)
    lv[0] = 2 if lv[0] == 1 else 1
    with pytest.raises(wc.WaveletError) as ei:
        ctx.thin_host(C.buf, C.off, C.units, C.n, lv, max_pairs=C.K if budget else None,
                      thresh=None if budget else C.thresh)
    assert ei.value.code == wc.capi.WC_ERR_FORMAT


def test_thinned_payloads_decode_on_the_device(wc, ctx):
    """wc_inverse_levels of the thinned payloads, where they lie, equals levels_ref.decode of the restatement's bytes."""
    import torch
    C = mixed(wc)
    d = Dev(wc, C, True)
    d.run(ctx)
    cells = torch.full((max(C.extent, 1),), -77.0, dtype=torch.float32, device=d.out.device)
    torch.cuda.synchronize()
    ctx.inverse_levels(d.out.data_ptr(), d.ooff.data_ptr(), C.units, C.n, C.levels, cells.data_ptr())
    ctx.synchronize()
    got = cells.cpu().numpy()
    for i, u in enumerate(C.us):
        o = C.units[i].cell_offset
        assert same_cells(got[o:o + u.N], R.decode(C.want[i][0])[0].ravel()), (i, u.name)


def test_thinning_the_full_payload_equals_the_budgeted_forward(wc, ctx):
    """On the device: wc_thin_budget(wc_forward_levels(thresh = 0), K) == wc_forward_levels_budget(K) byte for byte,
    with T and the thresholds, on fields without ties at the boundary (checked on the restatement)."""
    import torch
    spec = [((16, 16, 16), 4, 2), (BOX4, 3, 0), (BOX4, 1, 1), ((8, 8, 8), 2, 0), ((64, 32, 64), 3, 2)]
    dims = [s[0] for s in spec]
    levels = [s[1] for s in spec]
    boxes = [field(k, *d, seed=90 + i).astype(np.float32) for i, (d, _, k) in enumerate(spec)]
    units, n, extent = wc.capi.make_units(dims)
    K = [b.size // 4 + i for i, b in enumerate(boxes)]
    want = [BR.payload(b, L, k) for b, L, k in zip(boxes, levels, K)]
    assert all(w[4] == 1 for w in want)  # T's own candidate alone: no tie
    host = np.zeros(extent, np.float32)
    for i, b in enumerate(boxes):
        host[units[i].cell_offset:units[i].cell_offset + b.size] = b.ravel()
    dev = torch.device("cuda", 0)
    cells = torch.from_numpy(host).to(dev)
    cap = wc.capi.payload_bound(units, n)

    def bufs(cap):
        return (torch.full((cap,), 0xA5, dtype=torch.uint8, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev),
                torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros((n, WC_MAX_LEVELS), dtype=torch.float32, device=dev),
                torch.zeros(n, dtype=torch.int32, device=dev))

    full, direct = bufs(cap), bufs(cap)
    tcap = wc.capi.thin_bound(units, n, K)
    thin = bufs(tcap)
    torch.cuda.synchronize()
    ctx.forward_levels(cells.data_ptr(), wc.capi.WC_F32, units, n, levels, 0.0, 0.0, full[0].data_ptr(), cap,
                       full[1].data_ptr(), full[2].data_ptr())
    ctx.thin_budget(full[0].data_ptr(), full[1].data_ptr(), units, n, levels, K, thin[0].data_ptr(), tcap,
                    thin[1].data_ptr(), thin[2].data_ptr(), thin[3].data_ptr(), thin[4].data_ptr())
    ctx.forward_levels_budget(cells.data_ptr(), wc.capi.WC_F32, units, n, levels, K, direct[0].data_ptr(), cap,
                              direct[1].data_ptr(), direct[2].data_ptr(), direct[3].data_ptr(), direct[4].data_ptr())
    ctx.synchronize()

    def read(b):
        pay, off, kept = b[0].cpu().numpy(), b[1].cpu().numpy().view(np.uint64), b[2].cpu().numpy().view(np.uint32)
        return [wc.capi.unit_payload(pay, off, kept, i) for i in range(n)], kept, b[3].cpu().numpy(), b[4].cpu().numpy()

    tp, tk, tt, tkey = read(thin)
    dp, dk, dt, dkey = read(direct)
    for i in range(n):
        assert tp[i] == dp[i] == want[i][0], (i, dims[i], levels[i])
        assert int(tk[i]) == int(dk[i]) == want[i][1] and int(tkey[i]) == int(dkey[i]), i
    assert tt.tobytes() == dt.tobytes()
