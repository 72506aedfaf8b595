"""The size-budget mode without a GPU (include/wavelet_amd.h, wc_budget_select /
wc_budget_thresholds / wc_forward_levels_budget): the properties of the rule on
its numpy restatement (budget_rule.py), the host-only rule against the
restatement bit for bit, the proof that the GPU test's batch shows every class of
budget it claims, and the rule's translation unit under ASan + UBSan in a
stand-alone program (tests/cpp/test_budget.cpp)."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import budget_rule as BR
import leveltol_rule as LT
import levels_ref as R
import modes_batches as M
from tol_rule import HIST_SHIFT, field, same_bits

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "wavelet-compression_amd" / "csrc"
FIELDS = [((4, 4, 4), 2, 0), ((8, 8, 8), 3, 1), ((16, 16, 16), 4, 2), ((12, 20, 8), 2, 0), ((16, 16, 24), 1, 0),
          ((4, 2, 6), 1, 1), ((32, 16, 48), 4, 0), ((16, 16, 16), 3, 3)]
SPECIAL_TAGS = ("nan_first", "inf_pair", "inf_block", "plus_inf", "minus_inf", "neg_const")


def units():
    """(name, box fp32 [D, H, W], L): seeded fields, and the specials of modes_batches at 8^3, L = 1..3."""
    out = [((d, L, k), field(k, *d, seed=11 + i), L) for i, (d, L, k) in enumerate(FIELDS)]
    rng = np.random.default_rng(8400)
    for tag in SPECIAL_TAGS:
        for L in (1, 2, 3):
            b = M.special_box(tag, (8, 8, 8), rng).astype(np.float32)
            b.ravel()[rng.integers(0, b.size, 9)] = [0.0, -0.0, 1e-42, -1e-45, 0.0, 3e-39, np.float32(1e38), -0.0, 0.0]
            out.append(((tag, L), b, L))
    z = np.zeros((4, 4, 4), np.float32)
    z[1, 2, 3] = -0.0
    out.append((("zeros", 2), z, 2))
    return out


def budgets(c, rng):
    """Budgets around every edge of a unit with c candidates."""
    ks = {0, 1, c // 2, max(c - 1, 0), c, c + 1, c + 7, 0xFFFFFFFF}
    ks.update(int(v) for v in rng.integers(0, c + 1, 4))
    return sorted(ks)


def test_properties_of_the_rule():
    rng = np.random.default_rng(8401)
    for name, box, L in units():
        prep = BR.prepare(box, L)
        W, H, D, _, flat, k, cand, ks, _ = prep
        c = len(ks)
        assert c == int(cand.sum()) and (c == 0 or ks.max() <= 0x81C00000)
        everything = R.payload(box, L, thresh=0.0)
        last = -1
        for K in budgets(c, rng):
            pay, kept, T, th, ties = BR.payload_of(prep, K)
            who = (name, K, c)
            assert kept <= K, who
            if c > K:
                assert kept + ties >= K + 1 and ties >= 1 and T >= 1, who
            else:
                assert T == 0 and kept == c, who
                assert (pay, kept) == everything, who  # K >= candidates: wc_forward_levels with the explicit threshold 0.0f
            assert len(pay) == 20 + 8 * kept <= 20 + 8 * K, who
            # the mask by the per-level thresholds keeps exactly the candidates with key > T
            m = LT.mask(flat, W, H, D, L, th)
            assert np.array_equal(m.view(np.uint32) != 0, cand & (k > T)), who
            assert np.array_equal(m.view(np.uint32)[m.view(np.uint32) != 0], flat.view(np.uint32)[cand & (k > T)]), who
            assert kept >= last, who  # monotone in K
            last = kept
            if K == 0:
                assert kept == 0 and len(pay) == 20, who


def test_thresholds_at_the_edges_of_the_key_range():
    step = BR.level_step
    assert BR.thresholds(0, 4) == [0.0] * 4
    assert 0x7F800000 + step(4) == 0x81C00000
    th = BR.thresholds(0x81C00000, 4)
    assert all(np.isinf(t) and t > 0 for t in th)
    th = BR.thresholds(step(2), 2)  # level 2 at its offset exactly: d = 0
    assert th[1] == 0.0 and same_bits(th[0], BR.f32_from_bits(step(2)), np.float32)
    th = BR.thresholds(step(2) + 1, 2)
    assert same_bits(th[1], BR.f32_from_bits(1), np.float32)
    th = BR.thresholds(0x7F800000 + step(2) - 1, 2)
    assert np.isinf(th[0]) and same_bits(th[1], BR.f32_from_bits(0x7F7FFFFF), np.float32)


def test_host_rule_equals_the_restatement(wc):
    rng = np.random.default_rng(8402)
    for name, box, L in units():
        prep = BR.prepare(box, L)
        W, H, D, _, flat, _, _, ks, _ = prep
        for K in budgets(len(ks), rng):
            _, kept, T, th, _ = BR.payload_of(prep, K)
            gT, gth, gkept = wc.capi.budget_select(flat, (W, H, D), L, K)
            assert (gT, gkept) == (T, kept), (name, K, gT, T, gkept, kept)
            assert len(gth) == L and all(same_bits(a, b, np.float32) for a, b in zip(gth, th)), (name, K, gth, th)
            assert all(same_bits(a, b, np.float32) for a, b in zip(wc.capi.budget_thresholds(T, L), th)), (name, K)
    assert wc.capi.budget_select(np.zeros(0, np.float32), (0, 8, 8), 2, 5) == (0, [0.0, 0.0], 0)
    for bad in (lambda: wc.capi.budget_select(np.zeros(64, np.float32), (4, 4, 4), 3, 1),
                lambda: wc.capi.budget_select(np.zeros(64, np.float32), (4, 4, 4), 0, 1),
                lambda: wc.capi.budget_thresholds(1, 5)):
        with pytest.raises(wc.WaveletError) as ei:
            bad()
        assert ei.value.code == wc.capi.WC_ERR_INVALID


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_gpu_batch_shows_every_class(wc, dtype):
    """The batch and seeds of test_gpu_budget.py: every class of budget occurs, and each chosen K has the
    property its class names (read off the restatement's results)."""
    B = BR.Batch(wc.capi, dtype)
    tiles = [-(-b.size // 4096) for b in B.boxes]
    assert max(tiles) > 64 and 64 in tiles  # a split unit at the default, and the solo limit itself
    seen = {}
    for j in range(BR.CALLS):
        for i in range(B.n):
            cl, K, L = B.shown[j][i], B.budgets[j][i], B.levels[i]
            _, kept, T, th, ties = B.want[j][i]
            ks, lv = B.prep[i][7], B.prep[i][8]
            c = len(ks)
            seen.setdefault(cl, []).append(i)
            who = (cl, i, B.dims[i], L, K, c)
            assert kept <= K, who
            ok = {"zero": K == 0 and kept == 0,
                  "all": K == c and kept == c and T == 0,
                  "over": K == c + 7 and kept == c and T == 0,
                  "all_but_one": K == c - 1 and T == int(ks[-1]) if c else False,
                  "tie": 0 < K < c and ks[K - 1] == ks[K] and kept < K and ties >= 2,
                  "low_00": T & 0x7F == 0 and T > 0,
                  "low_7f": T & 0x7F == 0x7F,
                  "mid_000": (T >> 7) & 0xFFF == 0 and T > 0,
                  "mid_fff": (T >> 7) & 0xFFF == 0xFFF,
                  "top_differs": 0 < K < c and ks[K - 1] >> HIST_SHIFT != ks[K] >> HIST_SHIFT,
                  "mid_differs": 0 < K < c and ks[K - 1] >> HIST_SHIFT == ks[K] >> HIST_SHIFT
                                 and ks[K - 1] >> 7 != ks[K] >> 7,
                  "cross_level": 0 < K < c and L >= 2 and ks[K - 1] >> HIST_SHIFT == ks[K] >> HIST_SHIFT
                                 and lv[K - 1] != lv[K] and ks[K - 1] != ks[K],
                  "last_zero": L >= 2 and th[L - 1] == 0.0 and th[0] > 0.0 and kept < c,
                  "inf": any(np.isinf(t) for t in th)}[cl]
            assert ok, who
    assert set(seen) == set(BR.CLASSES), sorted(set(BR.CLASSES) - set(seen))
    specials = [i for i, (_, _, what) in enumerate(BR.SPEC) if what in ("inf_pair", "minus_inf")]
    assert set(seen["inf"]) <= set(specials)
    assert B.levels[BR.ONE_LEVEL] == 1 and B.boxes[BR.ONE_LEVEL].size
    # the constant box: every candidate of a level ties, and the split unit and the solo limit get binding budgets
    const = [i for i, (_, _, what) in enumerate(BR.SPEC) if what == 3][0]
    assert any(B.shown[j][const] == "tie" or 0 < B.budgets[j][const] < len(B.prep[const][7]) for j in range(BR.CALLS))
    for i in (tiles.index(max(tiles)), tiles.index(64)):
        assert sum(0 < B.budgets[j][i] < len(B.prep[i][7]) for j in range(BR.CALLS)) >= 3, i


def test_host_rule_under_sanitizer(tmp_path):
    """wc_budgetrule.cpp alone in tests/cpp/test_budget.cpp, built with ASan + UBSan
    (`make budgetsan`), on a table from the restatement: exactly W*H*D coefficients
    and L thresholds per case on the heap, so a read or write past either is
    reported.  Nothing is loaded into this process."""
    subprocess.run(["make", "-s", "-C", str(CSRC), "budgetsan"], check=True, timeout=600)
    rng = np.random.default_rng(8403)
    lines = []
    for name, box, L in units():
        if box.size > 4096:
            continue
        prep = BR.prepare(box, L)
        W, H, D, _, flat, _, _, ks, _ = prep
        body = " ".join(f"{int(v):x}" for v in flat.view(np.uint32))
        for K in budgets(len(ks), rng):
            _, kept, T, th, _ = BR.payload_of(prep, K)
            tb = " ".join(f"{int(np.array([x], np.float32).view(np.uint32)[0]):x}" for x in th)
            lines.append(f"{W} {H} {D} {L} {K} {T:x} {kept} {tb} {body}")
    lines.append("0 8 8 2 5 0 0 0 0 ")
    table = tmp_path / "budget_table.txt"
    table.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0:exitcode=66",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=66")
    r = subprocess.run([str(ROOT / "tools" / "bin" / "asan" / "test_budget"), str(table)], capture_output=True,
                       text=True, timeout=600, env=env)
    text = r.stdout + r.stderr
    assert "Sanitizer" not in text and "runtime error:" not in text, text[-4000:]
    assert r.returncode == 0 and f"{len(lines)} cases" in r.stdout and " 0 failed" in r.stdout, text[-4000:]
