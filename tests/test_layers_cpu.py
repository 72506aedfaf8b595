"""Progressive layers without a GPU (include/wavelet_amd.h, wc_split_unit /
wc_merge_unit): the host rule against the numpy restatement (layers_rule.py) byte
for byte, the identities the header states, and the refusals.

Inputs, as test_thin_cpu.py's: the thresh = 0 payloads of budget_rule.SPEC's boxes
at every L they admit, one odd-dimension box at L = 1, and the crafted units of
decode_payloads (surplus pairs, overshooting run sums past 2^31 - 1 and 2^32,
values +-0, NaN, +-inf, subnormals).  Budgets per unit: 0, 1, c - 1, c, c + 1, a tie
and a uniform rank (thin_rule.budgets), and the thresholds of each T."""
import numpy as np
import pytest

import decode_payloads as DP
import layers_rule as LR
import thin_rule as TR
from test_thin_cpu import CLASSES, all_payloads, crafted_units, field_units
from tol_rule import same_bits


def test_split_and_merge_equal_the_restatement_and_every_class_occurs(wc):
    capi = wc.capi
    rng = np.random.default_rng(9301)
    seen = {c: 0 for c in CLASSES}
    encoder_made = {name for name, _, _, _ in field_units(wc)}
    for name, pay in all_payloads(wc):
        canon = LR.canon(pay)
        if name in encoder_made:
            assert canon == pay, name  # an encoder's payload is its own canonical form
        for cl, K in TR.budgets(pay, rng).items():
            who = (name, cl, K)
            wbase, wrest, kept, rpairs, T, th = LR.split_budget(pay, K)
            base, rest, gT, gth = capi.split_unit(pay, max_pairs=K)
            assert (base, rest, gT) == (wbase, wrest, T), who
            assert all(same_bits(float(a), b, np.float32) for a, b in zip(gth, th)), who
            assert base == TR.thin_budget(pay, K)[0] == capi.thin_unit(pay, max_pairs=K)[0], who
            assert kept + rpairs == (len(canon) - 20) // 8, who
            # the identity, both orders, against the restatement and the canonical form
            assert capi.merge_unit(base, rest) == capi.merge_unit(rest, base) == LR.merge(base, rest) == canon, who
            # the threshold form at the thresholds of T gives the same layers
            tb, tr_, tk, trp = LR.split_thresh(pay, th)
            assert (tb, tr_) == (wbase, wrest), who
            assert capi.split_unit(pay, thresh=th)[:2] == (wbase, wrest), who
            # the next layer: three layers merged in both groupings
            b2, r2, _, _ = capi.split_unit(rest, max_pairs=rpairs // 2)
            assert (b2, r2) == LR.split_budget(rest, rpairs // 2)[:2], who
            left = capi.merge_unit(capi.merge_unit(base, b2), r2)
            right = capi.merge_unit(base, capi.merge_unit(b2, r2))
            assert left == right == canon, who
            seen[cl] += 1
    assert all(seen[c] > 0 for c in CLASSES), seen
    tags = set()
    for u in crafted_units():
        tags |= set(DP.classify(u))
        tags |= {"surplus"} if DP.is_surplus(u) else set()
        tags |= {"overshoot"} if DP.is_overshoot(u) else set()
    assert {"surplus", "overshoot", "val:specials", "val:nan", "val:+0", "val:-0-blocks"} <= tags, sorted(tags)
    sums = [int(np.asarray(u.runs, np.int64).sum()) + u.runs.size for u in crafted_units()]
    assert any(s > 2 ** 31 - 1 for s in sums) and any(s > 2 ** 32 for s in sums)


def test_merge_keeps_value_bits_verbatim_and_drops_only_what_lies_past_the_box(wc):
    """merge(a, empty) = a without its pairs past N: +-0 and NaN stay, unlike in canon(a)."""
    capi = wc.capi
    kinds = set()
    for u in crafted_units():
        W, H, D, nc, pos, bits = LR.live_pairs(u.payload)
        empty = LR.emit(W, H, D, nc, [], [])
        got = capi.merge_unit(u.payload, empty)
        assert got == capi.merge_unit(empty, u.payload) == LR.merge(u.payload, empty) == LR.emit(W, H, D, nc, pos, bits), u.name
        assert len(got) <= 20 + 8 * min(W * H * D, u.runs.size), u.name
        kinds |= {"dropped"} if pos.size < u.runs.size else set()
        kinds |= {"specials"} if pos.size and not LR.candidates(bits).all() else set()
        # split the live pairs by parity of their index: two interleaved layers, adjacent positions across the sources
        a = LR.emit(W, H, D, nc, pos[0::2], bits[0::2])
        b = LR.emit(W, H, D, nc, pos[1::2], bits[1::2])
        assert capi.merge_unit(a, b) == capi.merge_unit(b, a) == got, u.name
    assert kinds == {"dropped", "specials"}


def test_refusals(wc):
    capi = wc.capi
    _, _, _, pay = field_units(wc)[0]
    L = capi.payload_levels(pay[:20])
    base, rest, _, _ = capi.split_unit(pay, max_pairs=((len(pay) - 20) // 8) // 2)
    nb, nr = (len(base) - 20) // 8, (len(rest) - 20) // 8
    assert nb >= 3 and nr >= 3

    def code(f):
        with pytest.raises(wc.WaveletError) as ei:
            f()
        return ei.value.code

    INVALID, FORMAT = capi.WC_ERR_INVALID, capi.WC_ERR_FORMAT
    assert code(lambda: capi.split_unit(pay)) == INVALID                                   # neither form
    assert code(lambda: capi.split_unit(pay, max_pairs=1, thresh=[0.0] * L)) == INVALID    # both
    assert code(lambda: capi.split_unit(pay, thresh=[np.nan] * L)) == INVALID
    assert code(lambda: capi.split_unit(pay, thresh=[-1.0] * L)) == INVALID
    assert code(lambda: capi.split_unit(pay[:len(pay) - 8], max_pairs=1)) == INVALID       # short input
    assert code(lambda: capi.merge_unit(base[:len(base) - 8], rest)) == INVALID
    # short output buffers, either side
    assert code(lambda: capi.split_unit(pay, max_pairs=nb, base_cap=len(base) - 1)) == INVALID
    assert code(lambda: capi.split_unit(pay, max_pairs=nb, rest_cap=len(rest) - 1)) == INVALID
    assert capi.split_unit(pay, max_pairs=nb, base_cap=len(base), rest_cap=len(rest))[:2] == (base, rest)
    assert code(lambda: capi.merge_unit(base, rest, cap=len(pay) - 1)) == INVALID
    assert capi.merge_unit(base, rest, cap=len(pay)) == pay
    # a negative run, a header that is no standard one, a packed unit
    neg = bytearray(pay)
    neg[28:32] = np.array([-1], "<i4").tobytes()
    assert code(lambda: capi.split_unit(bytes(neg), max_pairs=1)) == FORMAT
    assert code(lambda: capi.merge_unit(bytes(neg), rest)) == FORMAT
    assert code(lambda: capi.merge_unit(rest, bytes(neg))) == FORMAT
    packed = capi.pack_unit(pay, 2)
    assert code(lambda: capi.split_unit(packed, max_pairs=1)) == FORMAT
    assert code(lambda: capi.merge_unit(packed, rest)) == FORMAT
    hdr = bytearray(base)
    hdr[12:16] = np.array([-9], "<i4").tobytes()  # no level count
    assert code(lambda: capi.merge_unit(bytes(hdr), rest)) == FORMAT
    # headers that differ: another level count, another box
    W, H, D, Lp, nc, _, _ = TR.parse(base)
    other = bytearray(base)
    other[12:16] = np.array([-2 if Lp != 2 else -3], "<i4").tobytes()
    assert code(lambda: capi.merge_unit(bytes(other), rest)) == FORMAT
    other = bytearray(base)
    other[0:8] = np.array([H, W], "<i4").tobytes() if W != H else np.array([W * 2, H // 2], "<i4").tobytes()
    assert code(lambda: capi.merge_unit(bytes(other), rest)) == FORMAT
    # an overlap at the first, a middle and the last pair
    _, _, _, _, bpos, bbits = LR.live_pairs(base)
    _, _, _, _, rpos, rbits = LR.live_pairs(rest)
    for at in (0, nb // 2, nb - 1):
        pos = np.sort(np.concatenate([rpos, bpos[at:at + 1]]))
        clash = LR.emit(W, H, D, nc, pos, np.resize(rbits, pos.size))
        assert code(lambda: capi.merge_unit(base, clash)) == FORMAT, at
        assert code(lambda: capi.merge_unit(clash, base)) == FORMAT, at
        with pytest.raises(LR.Overlap):
            LR.merge(base, clash)
    # +inf is a threshold: the base is empty, the rest is everything
    b, r, _, _ = capi.split_unit(pay, thresh=[np.inf] * L)
    assert len(b) == 20 and r == pay and (b, r) == LR.split_thresh(pay, [np.inf] * L)[:2]
