"""The pointwise (max-abs) error bound without a GPU (include/wavelet_amd.h,
wc_maxerr_select / wc_forward_levels_maxerr): the host-only rule against the
numpy restatement (maxerr_rule.py) bit for bit, the properties of the rule, the
payload at the found threshold, and the box on which err(b) is not monotone, so
that the leading run of the search and "the largest passing b" part ways."""
import json
import math
from pathlib import Path

import numpy as np
import pytest

import levels_ref as R
import maxerr_rule as MR
import modes_batches as M
from tol_rule import field, same_bits

GOLDEN = Path(__file__).resolve().parent / "golden" / "maxerr_nonmonotone.json"
FIELDS = [((2, 2, 2), 1, 1), ((4, 4, 4), 2, 0), ((8, 8, 8), 3, 1), ((16, 16, 16), 4, 2), ((12, 20, 8), 2, 0),
          ((16, 16, 24), 1, 0), ((4, 2, 6), 1, 1), ((32, 16, 48), 4, 0), ((16, 16, 16), 3, 3)]
SPECIAL_TAGS = ("nan_first", "inf_pair", "inf_block", "plus_inf", "minus_inf", "neg_const")


def nonmonotone_box():
    g = json.loads(GOLDEN.read_text())
    assert g["dims_whd"] == [4, 4, 4] and g["levels"] == 2
    return np.array(g["cells"], np.float32)


def units():
    """(name, box [D, H, W] in fp32 or fp64, L): seeded fields in both cell types, the
    specials of modes_batches at 8^3, the non-monotone box."""
    out = []
    for i, (d, L, k) in enumerate(FIELDS):
        f = field(k, *d, seed=31 + i)
        out.append(((d, L, k, "f32"), f, L))
        if i % 2 == 0:  # fp64 cells: the error is against the cells before narrowing
            g = f.astype(np.float64) * (1.0 + 2.0 ** -30)
            out.append(((d, L, k, "f64"), g, L))
    rng = np.random.default_rng(9100)
    for tag in SPECIAL_TAGS:
        for L in (1, 2):
            out.append(((tag, L), M.special_box(tag, (8, 8, 8), rng).astype(np.float32), L))
    out.append((("nonmonotone", 2), nonmonotone_box(), 2))
    return out


def bounds(x):
    f = np.abs(np.asarray(x, np.float64))
    f = f[np.isfinite(f)]
    m = float(f.max()) if f.size else 1.0
    return [0.0, math.inf, 1e-9 * m, 1e-1 * m, 1e-2 * m, 1e-3 * m]


def test_host_rule_equals_the_restatement(wc):
    for name, x, L in units():
        D, H, W = x.shape
        flat = R.decompose(x.astype(np.float32), L)
        for E in bounds(x):
            t, e, b = MR.select(x, L, E)
            gt, ge, gb = wc.capi.maxerr_select(flat, x, (W, H, D), L, E)
            who = (name, E)
            assert gb == b, (who, gb, b)
            assert same_bits(gt, float(t), np.float32), (who, gt, t)
            assert same_bits(ge, e), (who, ge, e)


def test_properties_of_the_rule():
    for name, x, L in units():
        u = MR.Unit(x, R.decompose(x.astype(np.float32), L), L)
        for E in bounds(x):
            b = MR.search(u, E)
            who = (name, E, b)
            if b > 0:
                assert u.err(b) <= E, who
            if E == math.inf:
                assert b == 4095 and MR.thr(b) == np.float32(MR.FLT_MAX), who
            if E == 0.0 and np.isfinite(x).all() and name[0] != "nonmonotone" and name[2:3] != (3,):
                # a finite box that is not exactly representable by its own pyramid: b* = 0 or err 0
                assert b == 0 or u.err(b) == 0.0, who
        # thr(b) keeps exactly the bins >= b
        for b in (1, 2, 0x3F8, 0xFEF):
            t = MR.thr(b)
            assert (int(np.array([t], np.float32).view(np.uint32)[0]) + 1) >> MR.SHIFT == b
        assert MR.thr(0) == 0.0 and MR.thr(0xFF0) == MR.thr(4095) == np.float32(MR.FLT_MAX)


def test_zero_bound_keeps_everything_on_noise():
    x = field(1, 8, 8, 8, seed=77)
    assert MR.select(x, 3, 0.0)[2] == 0
    assert MR.payload(x, 3, 0.0)[0] == R.payload(x, 3, thresh=0.0)[0]


def test_payload_is_levels_ref_at_the_found_threshold(wc):
    for name, x, L in units():
        D, H, W = x.shape
        b32 = x.astype(np.float32)
        for E in bounds(x)[3:5]:
            pay, kept, t, e, b = MR.payload(x, L, E)
            assert (pay, kept) == R.payload(b32, L, thresh=float(MR.thr(b)))
            assert wc.capi.payload_levels(pay[:20]) == L
            # the decode of those bytes is R_b: the promised error is the decoded one
            if np.isfinite(x).all():
                rec, _ = R.decode(pay)
                assert same_bits(MR.max_abs(x, rec), e), (name, E)
                assert b == 0 or MR.max_abs(x, rec) <= E
    empty = np.zeros((8, 8, 0), np.float32)
    pay, kept, t, e, b = MR.payload(empty, 2, 0.5)
    assert kept == 0 and float(t) == 0.0 and e == 0.0 and b == 0


def test_the_leading_run_is_the_definition_where_err_is_not_monotone(wc):
    """The first 4x4x4 box of integers in -8..8 that default_rng(7) draws, at L = 2:
    err(2054) = 10.875 and err(2056) = 8.125, a decreasing step.  Under E = 9 every
    probe of the radix-16 search passes (the all-dropped reconstruction is off by
    max|x| = 8 <= 9), so the search and "the largest passing b" both end at 4095
    although b = 2054 fails in between.  Under E = 8 they part: the probes stop at
    b* = 2044 (err 6.75) while b = 4095 passes too (err 8.0)."""
    x = nonmonotone_box()
    flat = R.decompose(x, 2)
    u = MR.Unit(x, flat, 2)
    assert u.err(2054) == 10.875 and u.err(2056) == 8.125
    largest = lambda E: max(b for b in range(4096) if u.err(b) <= E)  # noqa: E731
    assert MR.search(u, 9.0) == 4095 == largest(9.0) and not u.err(2054) <= 9.0
    assert MR.search(u, 8.0) == 2044 and u.err(2044) == 6.75
    assert largest(8.0) == 4095 and u.err(4095) == 8.0
    for E, b in ((9.0, 4095), (8.0, 2044)):
        gt, ge, gb = wc.capi.maxerr_select(flat, x, (4, 4, 4), 2, E)
        assert gb == b and same_bits(gt, float(MR.thr(b)), np.float32) and same_bits(ge, u.err(b))


def test_refusals_of_the_host_rule(wc):
    x = np.ones((2, 2, 2), np.float32)
    for dims, L, E in (((2, 2, 2), 1, math.nan), ((2, 2, 2), 1, -0.5), ((2, 2, 2), 0, 1.0), ((2, 2, 2), 5, 1.0),
                       ((2, 2, 2), 2, 1.0)):
        with pytest.raises(wc.WaveletError) as ei:
            wc.capi.maxerr_select(x, x, dims, L, E)
        assert ei.value.code == wc.capi.WC_ERR_INVALID
    assert wc.capi.maxerr_select(np.zeros(0, np.float32), np.zeros(0, np.float32), (0, 4, 4), 2, 1.0) == (0.0, 0.0, 0)
