"""RMSE tolerance on the multi-level transform without a GPU
(include/wavelet_amd.h, wc_tol_levels_threshold / wc_forward_levels_tol): the
host-only per-level selection rule against its numpy restatement
(leveltol_rule.py), bit for bit in every threshold and in the bound; with one
level it is wc_tol_threshold; the rule end to end through the restatements
(levels_ref + the oracle: transform, level bins, thresholds, masked payload,
reconstruction: the actual RMSE stays within the tolerance); the purpose (more
levels keep fewer pairs at the same tolerance); and the rule's translation unit
under ASan + UBSan in a stand-alone program (tests/cpp/test_leveltol.cpp)."""
import math
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import leveltol_rule as LT
import levels_ref as R
from tol_rule import FLT_MAX, HIST_BINS, MARGIN, field, same_bits, tol_rule

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "wavelet-compression_amd" / "csrc"
TOLS = (0.0, 1e-30, 1e-12, 1e-3, 1e-2, 0.1, 1.0, 3.7, 100.0, 1e6, 1e30, math.inf)
# The keep-everything round trip of every end-to-end input stays within this
# (fp32 rounding alone, |x| <= 8, up to four levels): MARGIN times the smallest
# tolerance whose actual RMSE is checked, so actual <= model + rounding <= tol *
# (1 + MARGIN) by the triangle inequality.  The one-level FLOOR of tol_rule.py
# (5e-7) does not carry over: 5.93e-7 at 4^3, kind 0, L = 2.
LEVEL_FLOOR = 1e-6
E2E = [((4, 4, 4), 2), ((8, 8, 8), 3), ((16, 16, 16), 4), ((32, 16, 48), 4)]
E2E_TOLS = (1e-3, 1e-2, 0.1, 1.0, 100.0)
assert LEVEL_FLOOR <= MARGIN * min(E2E_TOLS) * (1 + 1e-12)


def check(wc, counts, L, ncoeff, tol):
    got_t, got_b = wc.capi.tol_levels_threshold(counts, L, ncoeff, tol)
    want_t, want_b, stop = LT.pick(counts, L, ncoeff, tol)
    assert len(got_t) == L
    for l in range(L):
        assert same_bits(got_t[l], want_t[l], np.float32), (L, tol, l + 1, got_t, want_t)
    assert same_bits(got_b, want_b), (L, tol, got_b, want_b)
    assert got_b <= tol
    return got_t, got_b, stop


def random_counts(rng, L):
    """Sparse and dense level-major counts for L levels."""
    cases = []
    for _ in range(3):  # sparse
        h = np.zeros((L, HIST_BINS), np.uint64)
        for l in range(L):
            idx = rng.integers(0, HIST_BINS, 30)
            h[l, idx] = rng.integers(1, 10 ** 6, 30).astype(np.uint64)
        cases.append(h)
    for _ in range(2):  # dense over the finite range of ordinary data, level l holding about 8^-(l-1) of it
        h = np.zeros((L, HIST_BINS), np.uint64)
        for l in range(L):
            h[l, 700:1100] = rng.integers(0, max(2, 5000 >> (3 * l)), 400).astype(np.uint64)
        h[0, 0] = 12345
        cases.append(h)
    cases.append(rng.integers(1, 50, (L, HIST_BINS)).astype(np.uint64))  # every bin of every level
    return cases


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_host_rule_matches_restatement(wc, L):
    rng = np.random.default_rng(40 + L)
    for h in random_counts(rng, L):
        n = int(h.sum())
        for tol in TOLS:
            check(wc, h, L, n, tol)


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_host_rule_special_counts(wc, L):
    empty = np.zeros((L, HIST_BINS), np.uint64)
    for tol in TOLS:
        assert check(wc, empty, L, 0, tol)[:2] == ([FLT_MAX] * L, 0.0)   # N = 0: nothing to keep
        assert check(wc, empty, L, 64, tol)[:2] == ([FLT_MAX] * L, 0.0)  # every coefficient NaN: not counted
    for lev in range(L):
        for b in (0, 0xFEF, 0xFF0):  # zeros / tiny denormals, the last finite bin, +-inf: alone at one level
            h = empty.copy()
            h[lev, b] = 7
            for tol in TOLS:
                t, bound, stop = check(wc, h, L, 7, tol)
                if stop is not None:
                    assert stop == (b + LT.LTOL_SHIFT * lev, lev + 1)
                    # the stopping level keeps the bin, every level before it has dropped its own bin of that s
                    assert same_bits(t[lev], LT.bin_threshold(b), np.float32)
        h = empty.copy()
        h[lev, 0], h[lev, 0xFEF], h[lev, 0xFF0] = 5, 2, 1
        assert check(wc, h, L, 8, 0.0)[0][lev] == 0.0                     # tol 0: every non-zero coefficient kept
        t, bound, stop = check(wc, h, L, 8, math.inf)                     # tol inf: only +-inf survives
        assert t == [FLT_MAX] * L and bound == math.inf and stop is None


def test_host_rule_stops_at_every_level(wc):
    """A stop at l* = 1, at l* = L and in between: the same bin s of every level is
    populated, so the walk passes level 1, 2, ... of that s in turn and the
    tolerance decides where it ends."""
    L, b0 = 4, 1000
    h = np.zeros((L, HIST_BINS), np.uint64)
    for l in range(L):
        h[l, b0 - LT.LTOL_SHIFT * l] = 3  # all at s = b0
    n = int(h.sum())
    hi = [float(np.array([(b0 - LT.LTOL_SHIFT * l + 1) << 19], np.uint32).view(np.float32)[0]) for l in range(L)]
    terms = [3.0 * (float(8 ** (l + 1)) * (hi[l] * hi[l])) for l in range(L)]
    seen = set()
    for k in range(L + 1):
        # a budget between the sum of the first k terms and the next one
        lo = sum(terms[:k])
        budget = lo + 0.5 * terms[k] if k < L else 2.0 * lo
        t, bound, stop = check(wc, h, L, n, math.sqrt(budget / n))
        seen.add(None if stop is None else stop[1])
        if stop is not None:
            assert stop == (b0, k + 1)
            for l in range(L):  # levels before l* dropped their bin, the others keep it
                want = b0 - LT.LTOL_SHIFT * l + (1 if l < k else 0)
                assert same_bits(t[l], LT.bin_threshold(want), np.float32)
    assert seen == {1, 2, 3, 4, None}


def test_one_level_is_wc_tol_threshold(wc):
    rng = np.random.default_rng(9)
    for h in random_counts(rng, 1):
        n = int(h.sum())
        for tol in TOLS:
            t1, b1 = wc.capi.tol_threshold(h.reshape(-1), n, tol)
            tl, bl = wc.capi.tol_levels_threshold(h, 1, n, tol)
            want_t, want_b = tol_rule(h.reshape(-1), n, tol)
            assert same_bits(tl[0], t1, np.float32) and same_bits(bl, b1)
            assert same_bits(tl[0], want_t, np.float32) and same_bits(bl, want_b)


def test_host_rule_rejects_bad_arguments(wc):
    h = np.ones((2, HIST_BINS), np.uint64)
    for bad in (math.nan, -1.0, -0.5e-300, -math.inf):
        with pytest.raises(wc.WaveletError) as ei:
            wc.capi.tol_levels_threshold(h, 2, 2 * HIST_BINS, bad)
        assert ei.value.code == wc.capi.WC_ERR_INVALID
    for bad in (0, -1, wc.capi.WC_MAX_LEVELS + 1):
        with pytest.raises(wc.WaveletError) as ei:
            wc.capi.tol_levels_threshold(h, bad, 2 * HIST_BINS, 1.0)
        assert ei.value.code == wc.capi.WC_ERR_INVALID


@pytest.mark.parametrize("dims,L", E2E)
def test_rule_end_to_end_on_the_restatements(wc, oracle, dims, L):
    """decompose (L levels) -> level bins -> wc_tol_levels_threshold -> masked
    payload -> reconstruction: the model RMSE (weights 8^lvl, in double) is within
    the bound, the bound within the tolerance, and the actual RMSE within tol *
    (1 + MARGIN); the margin covers the fp32 rounding of the round trip, which is
    first confirmed for each input (keep-everything RMSE <= LEVEL_FLOOR)."""
    W, H, D = dims
    lvl = LT.level_map(W, H, D, L).reshape(-1)
    for kind in range(4):
        box = field(kind, W, H, D, seed=11 + kind)
        assert np.abs(box).max() <= 8.0
        floor = oracle.rmse(box, R.decode(R.payload(box, L, thresh=-1.0)[0])[0])
        print(f"dims {dims} L {L} kind {kind}: keep-everything RMSE {floor:.3g}")
        assert floor <= LEVEL_FLOOR, (dims, kind, floor)
        flat = R.decompose(box, L)
        counts = LT.level_counts(flat, W, H, D, L)
        for tol in E2E_TOLS:
            t, bound, _ = check(wc, counts, L, flat.size, tol)
            pay, kept, want_t, want_b, _, masked = LT.payload(box, L, tol)
            assert [np.float32(x).tobytes() for x in t] == [np.float32(x).tobytes() for x in want_t]
            dropped = (flat.astype(np.float64) - masked.astype(np.float64))
            model = math.sqrt(float(np.sum((8.0 ** lvl) * dropped * dropped)) / flat.size)
            assert model <= bound * (1 + 1e-12) + 1e-300, (dims, kind, tol, model, bound)
            assert bound <= tol
            got, gotL = R.decode(pay)
            assert gotL == L
            actual = oracle.rmse(box, got)
            print(f"  tol {tol:g}: kept {kept} bound {bound:.4g} model {model:.4g} actual {actual:.4g}")
            assert actual <= tol * (1 + MARGIN), (dims, kind, tol, actual)


def test_more_levels_keep_fewer_pairs(oracle):
    """The purpose: on the smooth 64^3 field at tol 1.0 three levels keep fewer
    pairs than one (578 against 8538 when this was written)."""
    box = field(0, 64, 64, 64, seed=11)
    kept = {L: LT.payload(box, L, 1.0)[1] for L in (1, 3)}
    print(f"64^3 kind 0, tol 1.0: kept pairs {kept}")
    assert kept[3] < kept[1]


def test_host_rule_under_sanitizer(tmp_path):
    """wc_leveltolrule.cpp alone in tests/cpp/test_leveltol.cpp, built with ASan +
    UBSan (`make leveltolsan`), on tables from the restatement: exactly L x 4096
    counts and L thresholds per case on the heap, so a read or write past either
    is reported.  Nothing is loaded into this process."""
    subprocess.run(["make", "-s", "-C", str(CSRC), "leveltolsan"], check=True, timeout=600)
    rng = np.random.default_rng(77)
    lines = []
    for L in (1, 2, 3, 4):
        cases = random_counts(rng, L)[::2]
        one = np.zeros((L, HIST_BINS), np.uint64)
        one[L - 1, 0xFF0], one[0, 0], one[L - 1, HIST_BINS - 1] = 2, 9, 1
        cases += [np.zeros((L, HIST_BINS), np.uint64), one]
        for h in cases:
            n = int(h.sum())
            flat = h.reshape(-1)
            nz = np.nonzero(flat)[0]
            body = " ".join(f"{int(i)} {int(flat[i])}" for i in nz)
            for tol in TOLS:
                t, b, _ = LT.pick(h, L, n, tol)
                tb = " ".join(f"{int(np.array([x], np.float32).view(np.uint32)[0]):x}" for x in t)
                lines.append(f"{L} {n} {int(np.array([tol], np.float64).view(np.uint64)[0]):x} "
                             f"{int(np.array([b], np.float64).view(np.uint64)[0]):x} {tb} {len(nz)} {body}")
    table = tmp_path / "leveltol_table.txt"
    table.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0:exitcode=66",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=66")
    r = subprocess.run([str(ROOT / "tools" / "bin" / "asan" / "test_leveltol"), str(table)], capture_output=True,
                       text=True, timeout=600, env=env)
    text = r.stdout + r.stderr
    assert "Sanitizer" not in text and "runtime error:" not in text, text[-4000:]
    assert r.returncode == 0 and f"{len(lines)} cases" in r.stdout and " 0 failed" in r.stdout, text[-4000:]
