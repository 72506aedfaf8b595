"""CPU: the seeded batches of tests/modes_batches.py hold what they claim, on the
restatements alone (levels_ref.py, coarse_ref.py, tol_rule.py, the oracle).

tests/test_gpu_modes_fuzz.py compares the device with these restatements on
these batches; a batch that silently lost its odd-hd chunk, its NaN at A[0] or
its inf - inf would let a wrong kernel pass.  So the conditions are proven
here, without a GPU, for the seeds the GPU tests run by default."""
import numpy as np
import pytest

import coarse_ref as C
import levels_ref as R
import modes_batches as M
from test_gpu_fuzz import same_cells
from tol_rule import tol_rule

LEVELS_SEEDS, COARSE_SEEDS, TOL_SEEDS = 4, 3, 3  # the K of each GPU test


def pairs(pay):
    return int(np.frombuffer(pay[16:20], "<i4")[0])


@pytest.fixture(scope="module")
def levels_batches(oracle):
    return [M.levels_batch(oracle, s) for s in range(LEVELS_SEEDS)]


def test_levels_batches_are_deterministic_and_within_their_caps(oracle, levels_batches):
    for s, B in enumerate(levels_batches):
        again = M.levels_batch(oracle, s)
        assert (again.dims, again.levels, again.offsets, again.extent, again.keep, again.tags) == \
            (B.dims, B.levels, B.offsets, B.extent, B.keep, B.tags)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again.boxes, B.boxes))
        assert B.dtype == (np.float64 if s % 2 == 0 else np.float32)
        assert 20 <= B.n <= 50 and len(B.dims) == len(B.levels) == len(B.boxes) == len(B.offsets) == B.n
        cells = [w * h * d for w, h, d in B.dims]
        assert max(cells) <= M.UNIT_CELLS and sum(cells) <= M.BATCH_CELLS
        assert all(x <= 128 for d in B.dims for x in d)
        assert 1 <= sum(c == 0 for c in cells) <= 2  # units without cells
        for (W, H, D), L, b in zip(B.dims, B.levels, B.boxes):
            assert b.shape == (D, H, W)
            assert 1 <= L <= R.levels_for(W, H, D, R.MAX_LEVELS), ((W, H, D), L)  # wc_levels_for's divisibility rule
        # packed in order with gaps, odd and even cell offsets both present
        end = 0
        for o, c in zip(B.offsets, cells):
            assert o >= end
            end = o + c
        assert B.extent == end
        assert any(o % 2 for o in B.offsets) and any(o % 2 == 0 for o in B.offsets)
        assert set(B.levels) == {1, 2, 3, 4}
        for i, (tag, d, L) in enumerate(M.PINNED + M.SPECIALS):
            assert B.tags[tag] == i and B.dims[i] == d and B.levels[i] == L
    # over the seeds: L = 1 units with odd dims, and axes with unequal 2-adic parts
    every = [(d, L) for B in levels_batches for d, L in zip(B.dims, B.levels)]
    assert any(L == 1 and all(x % 2 for x in d) for d, L in every)
    assert any(L >= 2 and len({x & -x for x in d}) == 3 for d, L in every)


def test_levels_pinned_shapes_reach_their_paths():
    """From the dims alone (wc_levels.hip: a workgroup takes 4096 blocks; odd hd
    takes the scalar branch of k_level and d % 4 == 2 the 8-B branch of k_level_copy)."""
    shapes = {t: (d, L) for t, d, L in M.PINNED}

    def last(tag):
        d, L = shapes[tag]
        hw, hh, hd = M.level_blocks(d, L)
        return hw * hh * hd, hd, d[2] >> (L - 1)

    assert last("l4_cube") == (1, 1, 2)
    assert last("l4_unequal") == (3 * 1 * 5, 5, 10)
    assert last("odd_hd_3072") == (3072, 3, 6)
    assert last("odd_hd_l3") == (16 * 16 * 3, 3, 6)
    nblk, hd, d = last("odd_hd_5120")
    assert nblk == 5120 > M.LV_BLOCKS and hd % 2 == 1
    nblk, hd, d = last("float2_copy")
    assert nblk == 4608 > M.LV_BLOCKS and d % 4 == 2
    # the even-hd branch over several chunks, at every level of one unit
    d, L = shapes["l3_cube"]
    assert [np.prod(M.level_blocks(d, l)) for l in (2, 3)] == [4096, 512] and M.level_blocks(d, 3)[2] % 2 == 0


def test_levels_special_units(oracle, levels_batches):
    for B in levels_batches:
        def unit(tag):
            i = B.tags[tag]
            return M.narrow(oracle, B.boxes[i], B.dtype), B.levels[i]
        # a NaN in cell (0, 0, 0) reaches A[0]: a NaN threshold, nothing kept at any keep
        b, L = unit("nan_first")
        flat = R.decompose(b, L)
        assert np.isnan(flat[0]) and np.isnan(b[0, 0, 0]) and np.isnan(b).sum() == 1
        for keep in (0.0, float(np.float32(0.999)), 1.5):
            assert R.payload(b, L, keep=keep)[1] == 0, keep
        # +inf and -inf in two level-1 blocks of one level-2 block: the NaN is made by the level pass
        b, L = unit("inf_pair")
        assert not np.isnan(b).any() and np.isinf(b).sum() == 2
        assert not np.isnan(oracle.wavelet_decompose(b)).any()
        flat = R.decompose(b, L)
        assert np.isnan(flat).any() and np.isinf(flat).any() and np.isfinite(flat[0])
        # ... and the synthesis meets inf - inf: keep 1.5 keeps every non-NaN coefficient (thresh -inf)
        pay, kept = R.payload(b, L, keep=1.5)
        assert kept == int((~np.isnan(flat)).sum()) > 0
        assert np.isnan(R.decode(pay)[0]).any()
        # a lone -inf: the first largest |c| is the low-pass -inf, so thresh = -inf (all) or +inf (none)
        b, L = unit("minus_inf")
        flat = R.decompose(b, L)
        assert not np.isnan(flat).any() and flat[np.isinf(flat)][0] == -np.inf
        assert R.payload(b, L, keep=float(np.float32(0.999)))[1] == b.size
        assert R.payload(b, L, keep=1.5)[1] == 0


def test_coarse_cases_decode_as_the_long_form(oracle, levels_batches):
    seen = set()
    for s in range(COARSE_SEEDS):
        B = levels_batches[s]
        pays, reduce, odd_at, surplus_at = M.coarse_cases(oracle, B, np.random.default_rng(7500 + s))
        again = M.coarse_cases(oracle, B, np.random.default_rng(7500 + s))
        assert (pays, reduce, odd_at, surplus_at) == again
        assert len(pays) == len(reduce) > B.n  # every unit, then the one-level oracle payloads
        assert len(surplus_at) == 3
        for i in surplus_at:
            W, H, D = B.dims[i]
            assert pairs(pays[i]) == W * H * D + 5
        for i in range(B.n, len(pays) - 5):
            assert C.payload_levels(pays[i]) == 1 and reduce[i] == 1
        assert [C.payload_levels(p) for p in pays[-5:]] == [4] * 5 and reduce[-5:] == [0, 1, 2, 3, 4]
        assert set(reduce) >= {0, 1, 2}
        for i, (p, r) in enumerate(zip(pays, reduce)):
            (W, H, D), L = tuple(int(x) for x in np.frombuffer(p[:12], "<i4")), C.payload_levels(p)
            assert 0 <= r <= L and (W * H * D == 0 or (W | H | D) & ((1 << r) - 1) == 0)
            if i < B.n:
                assert (W, H, D) == B.dims[i] and L == B.levels[i]
            got = C.decode(p, r)
            want = R.decode(p)[0] if r == 0 else C.long_form(p, r)
            assert same_cells(got.ravel(), want.ravel()), (s, i, (W, H, D), L, r)
            seen.add((L, r))
        assert C.coarse_dims(*np.frombuffer(pays[odd_at][:12], "<i4"), reduce[odd_at])[0] > 0
    # over the seeds: every r of every L, r == L (no arithmetic) and r < L (level passes on the corner)
    assert seen == {(L, r) for L in range(1, 5) for r in range(L + 1)}


def test_tol_batches(oracle):
    inf_bins = nan_coefs = inf_dropped = 0
    for s in range(TOL_SEEDS):
        B, again = M.tol_batch(oracle, s), M.tol_batch(oracle, s)
        assert (again.dims, again.offsets, again.extent) == (B.dims, B.offsets, B.extent)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again.boxes, B.boxes))
        assert np.array_equal(np.array(again.tol), np.array(B.tol))
        assert 20 <= B.n <= 60 and B.dims[:3] == [(64, 64, 64), (64, 64, 12), M.TOL_WIDE[1]]
        assert all(x in M.TOL_SIZES for d in B.dims for x in d)
        tiles = [-(-w * h * d // 4096) for w, h, d in B.dims]  # flat tiles: WC_OPT_TOL_SOLO_TILES = 1 splits >= 2
        assert any(t == 1 for t in tiles) and sum(t >= 2 for t in tiles) >= 2
        assert any(d[2] % 8 == 0 for d in B.dims) and any(d[2] % 8 for d in B.dims)
        assert all(t >= 0.0 for t in B.tol) and 0.0 in B.tol and np.inf in B.tol
        assert any(0.0 < t < np.inf for t in B.tol)
        for b, tol in zip(B.boxes, B.tol):
            with np.errstate(all="ignore"):
                flat = oracle.wavelet_decompose(M.narrow(oracle, b, B.dtype))
            counts = oracle.magnitude_hist(flat)
            thresh, bound = tol_rule(counts, flat.size, tol)
            assert bound <= tol or (np.isinf(bound) and np.isinf(tol)), (s, b.shape, tol, bound)
            assert thresh >= 0.0
            if b is B.boxes[M.TOL_WIDE[0]]:  # the wide-range unit: a finite sum of 10^60 and more
                assert np.isfinite(bound) and bound * bound * flat.size >= 1e60, (s, bound)
            if np.isinf(tol) and counts[0xFF0]:  # an inf bin under an infinite budget: dropped, but kept by FLT_MAX
                assert np.isinf(bound) and thresh == float(np.finfo(np.float32).max)
                inf_dropped += 1
            inf_bins += int(counts[0xFF0]) > 0
            nan_coefs += bool(np.isnan(flat).any())
    # the specials reach the rule: units with inf coefficients (the +inf bin) and with NaN ones
    assert inf_bins and nan_coefs and inf_dropped
