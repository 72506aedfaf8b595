"""CPU: the tolerance rule of the compressed-domain thinning and split on one payload
(include/wavelet_amd.h wc_thin_tol_unit / wc_split_tol_unit, plain C++) against the
numpy restatement (thin_tol_rule.py), which goes through the dense array A(P) where
the product counts the pairs.

Bar: bytes, thresholds (float bits) and bound (double bits) equal the restatement's;
on a thresh = 0 payload they equal wc_forward_levels_tol's restatement
(leveltol_rule.payload) at the same tolerance; merge(split_tol(P)) == canon(P);
successive thinnings stay within the root of the summed squared bounds."""
import math

import numpy as np
import pytest

import layers_rule as LR
import leveltol_rule as LT
import levels_ref as R
import pack_rule as PR
import thin_rule as TR
import thin_tol_rule as TT
from tol_rule import FLT_MAX, MARGIN, field

BOXES = [((16, 16, 16), 4, 0), ((32, 16, 32), 1, 1), ((32, 16, 32), 2, 2), ((32, 16, 32), 3, 0), ((48, 16, 80), 4, 2),
         ((8, 8, 8), 3, 1)]
FRACTIONS = (0.0, 1e-3, 0.01, 0.1, 0.5, 3.0, math.inf)
_memo = {}


def boxes():
    """[(box [D, H, W] float32, L, RMS, its thresh = 0 payload)]"""
    if "boxes" not in _memo:
        out = []
        for j, (dims, L, kind) in enumerate(BOXES):
            b = field(kind, *dims, seed=180 + j).astype(np.float32)
            out.append((b, L, float(np.sqrt(np.mean(b.astype(np.float64) ** 2))), R.payload(b, L, thresh=0.0)[0]))
        _memo["boxes"] = out
    return _memo["boxes"]


def same_outputs(got_th, got_bound, th, bound, L):
    return TT.th_bits(got_th) == TT.th_bits(th, L) and TT.f64_bits(got_bound) == TT.f64_bits(bound)


def test_the_batch_shows_what_it_claims():
    B = TT.batch()
    by = {u.name: i for i, u in enumerate(B.us)}
    assert sorted(u.pairs for u in B.us[:len(TT.COUNTS)]) == sorted(TT.COUNTS)
    stops = {w[4][1] for w in B.want if w[4] is not None}
    assert stops >= {1, 2, 3, 4}  # the walk stops at every level
    # a stop at l* >= 2 where the "+ 1 for l < l*" moves a threshold: level 1 keeps one bin less than level l* does
    moved = 0
    for u, w in zip(B.us, B.want):
        if w[4] is None or w[4][1] < 2:
            continue
        s, _ = w[4]
        if 0 < s + 1 < LT.HIST_BINS and TT.th_bits([w[2][0]]) != TT.th_bits([LT.bin_threshold(s)]):
            assert TT.th_bits([w[2][0]]) == TT.th_bits([LT.bin_threshold(s + 1)]), u.name
            moved += 1
    assert moved >= 3
    i = by["tol=0"]
    assert B.want[i][0] == LR.canon(B.us[i].payload) and B.want[i][4] == (0, 1) and B.want[i][3] == 0.0
    assert B.want[i][1] < B.us[i].pairs  # +-0 and NaN pairs leave
    i = by["tol=inf-finite"]
    assert B.want[i][1] == 0 and len(B.want[i][0]) == 20 and B.want[i][4] is None
    i = by["tol=inf"]  # the walk never stops: thresh_l = FLT_MAX keeps the +-inf pairs, as the forward does
    _, _, _, _, _, _, obits = TR.parse(B.want[i][0])
    assert sorted(obits.tolist()) == [0x7F800000, 0xFF800000] and all(t == FLT_MAX for t in B.want[i][2])
    for name in ("empty", "empty-L2"):
        assert B.want[by[name]][1] == 0 and B.want[by[name]][3] == 0.0
    # the zero count: the walk passes (0, 1) by half a coefficient; a NaN pair of level 1 counted in bin 0, or
    # left among the zeros, would stop it there
    i = by["zero-count"]
    u = B.us[i]
    W, H, D, L, _, runs, bits = TR.parse(u.payload)
    pos = np.cumsum(runs.astype(np.int64) + 1) - 1
    live = pos < u.N
    assert int((~live).sum()) == 5  # pairs past N
    lvl = LT.level_map(W, H, D, L).reshape(-1)
    m = bits & np.uint32(0x7FFFFFFF)
    nan1 = int(((m[live] > 0x7F800000) & (lvl[pos[live]] == 1)).sum())
    assert nan1 >= 1 and {0, 0x80000000, 0x7F800000, 0xFF800000} <= set(bits[live].tolist())
    assert ((m[live] > 0) & (m[live] < 0x00800000)).any()  # a subnormal
    tol, cnt = TT.zero_count_tol(u.payload)
    assert tol == u.tol and B.want[i][4] is not None and B.want[i][4] != (0, 1)
    N1 = u.N - (W >> 1) * (H >> 1) * (D >> 1)
    pairs1 = int((lvl[pos[live]] == 1).sum())
    bin0 = int(((m[live] <= 0x7F800000) & (m[live] >> LT.HIST_SHIFT == 0) & (lvl[pos[live]] == 1)).sum())
    assert cnt == N1 - pairs1 + bin0  # the issue's formula, NaN pairs among the pairs taken off
    counts = LT.level_counts(TR.dense(u.payload)[5], W, H, D, L)
    counts[0, 0] += 1
    assert LT.pick(counts, L, u.N, u.tol)[2] == (0, 1)
    assert {u.dims for u in B.us} >= {(16, 16, 16), TT.BOX4, TT.BOX15, TT.BOX72, (0, 4, 4)}
    assert {(u.dims, u.L) for u in B.us} >= {((16, 16, 16), 4), (TT.BOX4, 1), (TT.BOX4, 2), (TT.BOX4, 3), (TT.BOX15, 4)}
    assert all(w[3] <= u.tol for u, w in zip(B.us, B.want))  # bound <= tol


def test_unit_rule_matches_the_restatement(wc):
    B = TT.batch()
    for u, w, s in zip(B.us, B.want, B.split):
        out, th, bound = wc.capi.thin_tol_unit(u.payload, u.tol)
        assert out == w[0] and same_outputs(th, bound, w[2], w[3], u.L), u.name
        base, rest, th, bound = wc.capi.split_tol_unit(u.payload, u.tol)
        assert base == w[0] == s[0] and rest == s[1] and same_outputs(th, bound, w[2], w[3], u.L), u.name
        assert wc.capi.merge_unit(base, rest) == LR.canon(u.payload), u.name
        if u.box is not None:  # an encoder's payload is its own canonical form
            assert LR.canon(u.payload) == u.payload, u.name


def test_thinning_the_full_payload_equals_the_forward(wc):
    """thin_tol(thresh = 0 payload, tol) == leveltol_rule.payload(box, L, tol): bytes, thresholds, bound."""
    stops = set()
    for b, L, rms, full in boxes():
        for f in FRACTIONS:
            tol = f * rms if math.isfinite(f) else f
            pay, kept, th, bound, _, _ = LT.payload(b, L, tol)
            out, gth, gbound = wc.capi.thin_tol_unit(full, tol)
            assert out == pay and same_outputs(gth, gbound, th, bound, L), (b.shape, L, f)
            assert TT.thin_tol(full, tol)[0] == pay, (b.shape, L, f)  # and the restatement agrees with itself
            stop = TT.thresholds(full, tol)[2]
            stops.add(stop[1] if stop else None)
            if f == 0.0:
                assert out == full
            if not math.isfinite(f):
                assert kept == 0
    assert stops >= {1, 2, 3, 4, None}


def test_bounds_of_successive_thinnings_compose(wc):
    """A payload written at tol0 = 0.01 RMS and thinned at tol1 = 0.03 RMS decodes within
    sqrt(bound0^2 + bound1^2) (1 + MARGIN) of the box (tol_rule.MARGIN: the round trip's fp32 rounding)."""
    for b, L, rms, _ in boxes():
        pay0, _, _, bound0, _, _ = LT.payload(b, L, 0.01 * rms)
        out, _, bound1 = wc.capi.thin_tol_unit(pay0, 0.03 * rms)
        assert 0.01 * rms >= 1e-3 and bound1 <= 0.03 * rms
        got = R.decode(out)[0].astype(np.float64)
        rmse = float(np.sqrt(np.mean((got - b.astype(np.float64)) ** 2)))
        assert rmse <= math.sqrt(bound0 * bound0 + bound1 * bound1) * (1.0 + MARGIN), (b.shape, L, rmse, bound0, bound1)
        assert len(out) < len(pay0)


def test_refusals(wc):
    INVALID, FORMAT = wc.capi.WC_ERR_INVALID, wc.capi.WC_ERR_FORMAT
    B = TT.batch()
    u = B.us[{x.name: i for i, x in enumerate(B.us)}["L4"]]
    for bad in (math.nan, -1.0, -0.5):
        for call in (wc.capi.thin_tol_unit, wc.capi.split_tol_unit):
            with pytest.raises(wc.WaveletError) as ei:
                call(u.payload, bad)
            assert ei.value.code == INVALID
    odd = PR.standard(33, 17, 31, 1, np.array([5], np.uint32), np.float32(2.0).view(np.uint32).reshape(1))
    quarter = PR.standard(12, 8, 8, 3, np.array([5], np.uint32), np.float32(2.0).view(np.uint32).reshape(1))
    # a box wc_forward_levels_tol does not take: odd at L = 1; at L >= 2 the header itself is none (wc_payload_levels)
    for pay, code in ((odd, INVALID), (quarter, FORMAT)):
        with pytest.raises(wc.WaveletError) as ei:
            wc.capi.thin_tol_unit(pay, 0.5)
        assert ei.value.code == code
    with pytest.raises(wc.WaveletError) as ei:
        wc.capi.thin_tol_unit(wc.capi.pack_unit(u.payload, 3), 0.5)
    assert ei.value.code == FORMAT
    with pytest.raises(wc.WaveletError) as ei:  # a short output: nothing is written past it
        wc.capi.thin_tol_unit(u.payload, 0.0, cap=24)
    assert ei.value.code == INVALID
