"""Thinning in the compressed domain without a GPU (include/wavelet_amd.h,
wc_thin_unit): the host rule against the numpy restatement (thin_rule.py) byte
for byte, the identities the header states, and the refusals.

Inputs: the thresh = 0 payloads of budget_rule.SPEC's boxes at every L in 1..4
the box admits, one odd-dimension box at L = 1, and the crafted units of
decode_payloads (surplus pairs, overshooting run sums, values +-0, NaN, +-inf,
subnormals; none has a negative run).  Budgets per unit: 0, 1, kept - 1, kept,
kept + 1, a tie and a uniform rank (thin_rule.budgets), and the thresholds
wc_budget_thresholds gives for each T."""
import numpy as np
import pytest

import budget_rule as BR
import decode_payloads as DP
import levels_ref as R
import thin_rule as TR
from tol_rule import same_bits

CLASSES = ("zero", "one", "all_but_one", "all", "over", "tie", "rank")
_memo = {}


def field_units(wc):
    """[(name, box fp32 [D, H, W], L, thresh = 0 payload)]"""
    if "f" not in _memo:
        B = BR.Batch(wc.capi, np.float32)
        out = []
        boxes = [(B.dims[i], B.boxes[i], BR.SPEC[i][2]) for i in range(B.n)]
        odd = np.random.default_rng(9100).standard_normal((7, 5, 3)).astype(np.float32)  # [D, H, W]
        boxes.append(((3, 5, 7), odd, "odd"))
        for (W, H, D), b, what in boxes:
            for L in range(1, 5):
                if b.size and L >= 2 and (W | H | D) & ((1 << L) - 1):
                    continue
                if b.size > 65536 and L not in (1, 3):  # the large boxes: the one-level and one deep form
                    continue
                out.append((((W, H, D), L, what), b, L, R.payload(b, L, thresh=0.0)[0]))
        _memo["f"] = out
    return _memo["f"]


def crafted_units():
    return [u for u in DP.crafted() if u.runs.size == 0 or int(u.runs.max()) <= DP.M]


def all_payloads(wc):
    return [(name, pay) for name, _, _, pay in field_units(wc)] + [(u.name, u.payload) for u in crafted_units()]


def test_host_rule_equals_the_restatement_and_every_class_occurs(wc):
    rng = np.random.default_rng(9101)
    seen = {c: 0 for c in CLASSES}
    tags = set()
    for name, pay in all_payloads(wc):
        W, H, D, L, _, runs, bits = TR.parse(pay)
        for cl, K in TR.budgets(pay, rng).items():
            want, kept, T, th, ties = TR.thin_budget(pay, K)
            got, gT, gth = wc.capi.thin_unit(pay, max_pairs=K)
            who = (name, cl, K)
            assert got == want and gT == T, who
            assert all(same_bits(float(a), b, np.float32) for a, b in zip(gth, th)), who
            assert kept <= min(K, runs.size) and len(got) <= len(pay), who
            # the per-level thresholds of T keep the same set; both forms are idempotent
            tt, _ = TR.thin_thresh(pay, th)
            assert tt == want, who
            assert wc.capi.thin_unit(pay, thresh=th)[0] == want, who
            assert wc.capi.thin_unit(want, max_pairs=K)[0] == want, who
            assert wc.capi.thin_unit(want, thresh=th)[0] == want, who
            _, _, _, _, _, _, obits = TR.parse(want)
            m = obits & 0x7FFFFFFF
            assert ((m >= 1) & (m <= 0x7F800000)).all(), who  # no +-0, no NaN
            if cl == "tie":
                assert ties >= 2 and kept < K, who
            if cl == "zero":
                assert kept == 0 and len(got) == 20, who
            seen[cl] += 1
    for u in crafted_units():
        tags |= set(DP.classify(u))
        tags |= {"surplus"} if DP.is_surplus(u) else set()
        tags |= {"overshoot"} if DP.is_overshoot(u) else set()
    assert all(seen[c] > 0 for c in CLASSES), seen
    assert {"surplus", "overshoot", "val:specials", "val:nan", "val:+0", "val:-0-blocks"} <= tags, sorted(tags)


def test_thinning_a_field_payload_equals_the_forward(wc):
    """thresh = 0 payloads hold every candidate: a budget K gives budget_rule.payload(box, L, K), thresholds all
    equal to t1 >= t0 give wc_forward_levels' bytes at t1, and wc_budget_select on A(P) finds the same T."""
    rng = np.random.default_rng(9102)
    for name, box, L, pay in field_units(wc):
        W, H, D, _, _, flat = TR.dense(pay)
        prep = BR.prepare(box, L)
        for cl, K in TR.budgets(pay, rng).items():
            want = BR.payload_of(prep, K)
            got, gT, _ = wc.capi.thin_unit(pay, max_pairs=K)
            assert got == want[0] and gT == want[2], (name, cl, K)
            if flat.size and not (W | H | D) & 1:  # wc_budget_select wants even dimensions
                sT, _, skept = wc.capi.budget_select(flat, (W, H, D), L, K)
                assert (sT, skept) == (gT, want[1]), (name, cl, K)
        if not box.size:
            continue
        mags = np.abs(R.decompose(box, L))
        mags = mags[np.isfinite(mags)]
        t0 = float(np.quantile(mags, 0.3)) if mags.size else 0.0
        p0 = R.payload(box, L, thresh=t0)[0]
        for t1 in (t0, float(np.float32(t0 * 2 + 1e-3)), float(np.quantile(mags, 0.9)) if mags.size else 1.0, np.inf):
            if t1 < t0:
                continue
            assert wc.capi.thin_unit(p0, thresh=[t1] * L)[0] == R.payload(box, L, thresh=t1)[0], (name, t0, t1)


def test_refusals(wc):
    capi = wc.capi
    _, _, _, pay = field_units(wc)[0]
    L = capi.payload_levels(pay[:20])

    def code(f):
        with pytest.raises(wc.WaveletError) as ei:
            f()
        return ei.value.code

    assert code(lambda: capi.thin_unit(pay)) == capi.WC_ERR_INVALID                      # neither form
    assert code(lambda: capi.thin_unit(pay, max_pairs=1, thresh=[0.0] * L)) == capi.WC_ERR_INVALID  # both
    assert code(lambda: capi.thin_unit(pay, thresh=[np.nan] * L)) == capi.WC_ERR_INVALID
    assert code(lambda: capi.thin_unit(pay, thresh=[-1.0] * L)) == capi.WC_ERR_INVALID
    assert code(lambda: capi.thin_unit(pay[:len(pay) - 8], max_pairs=1)) == capi.WC_ERR_INVALID  # short
    neg = bytearray(pay)
    assert len(pay) >= 36
    neg[28:32] = np.array([-1], "<i4").tobytes()  # the second pair's run
    assert code(lambda: capi.thin_unit(bytes(neg), max_pairs=1)) == capi.WC_ERR_FORMAT
    packed = capi.pack_unit(pay, 2)
    assert code(lambda: capi.thin_unit(packed, max_pairs=1)) == capi.WC_ERR_FORMAT
    hdr = bytearray(pay)
    hdr[12:16] = np.array([-9], "<i4").tobytes()  # no level count
    assert code(lambda: capi.thin_unit(bytes(hdr), max_pairs=1)) == capi.WC_ERR_FORMAT
    # +inf is a threshold: nothing is kept
    out, _, _ = capi.thin_unit(pay, thresh=[np.inf] * L)
    assert len(out) == 20 and TR.thin_thresh(pay, [np.inf] * L)[0] == out
