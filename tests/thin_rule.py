"""Shared by the tests of the compressed-domain thinning (test_thin_cpu.py,
test_gpu_thin.py, test_gpu_thin_mirror.py): the numpy restatement of the rule
include/wavelet_amd.h documents for wc_thin_unit / wc_thin_budget /
wc_thin_thresh.  TEST INFRASTRUCTURE ONLY.

A(P) is the dense array the project's decode rule gives (exact positions from the
runs, decode_payloads.positions; pairs at or past N dropped).  The level and key of an entry are
budget_rule's and leveltol_rule's; the output is the oracle's RLE + serialize on
the kept set.  Only integers enter the budget form; the threshold form compares
float32 magnitudes."""
import numpy as np

import budget_rule as BR
import decode_payloads as DP
import leveltol_rule as LT
from oracle import oracle as O

MAX_LEVELS = 4
TILE = 4096


def parse(pay):
    """payload bytes -> (W, H, D, L, ncoeff field, runs uint32, value bits uint32)."""
    hdr = np.frombuffer(pay[:20], "<i4")
    W, H, D, nc, n = (int(x) for x in hdr)
    body = np.frombuffer(pay[20:20 + 8 * n], np.uint32).reshape(-1, 2)
    return W, H, D, (1 if nc >= 0 else -nc), nc, body[:, 0].copy(), body[:, 1].copy()


def dense(pay):
    """-> (W, H, D, L, ncoeff field, A(P) as float32 [N])."""
    W, H, D, L, nc, runs, bits = parse(pay)
    assert runs.size == 0 or int(runs.max()) <= DP.M, "a negative run has no A(P)"
    pos = DP.positions(runs)  # exact, strictly increasing
    live = pos < W * H * D
    flat = np.zeros(W * H * D, np.uint32)
    flat[pos[live]] = bits[live]
    return W, H, D, L, nc, flat.view(np.float32)


def _emit(W, H, D, nc, flat, keep):
    if flat.size == 0:
        return O.serialize(W, H, D, nc, [], []), 0
    m = np.where(keep, flat.view(np.uint32), np.uint32(0)).view(np.float32)
    runs, vals = O.threshold_rle(m, 0.0)
    assert len(runs) == int(keep.sum())
    return O.serialize(W, H, D, nc, runs, vals), len(runs)


def sorted_keys(pay):
    """The candidates' keys of A(P), descending (int64)."""
    W, H, D, L, _, flat = dense(pay)
    if flat.size == 0:
        return np.zeros(0, np.int64)
    return BR.sorted_keys(flat, W, H, D, L)[0]


def thin_budget(pay, K):
    """-> (bytes, kept, T, [thresh_1..L], ties)."""
    W, H, D, L, nc, flat = dense(pay)
    if flat.size == 0:
        return O.serialize(W, H, D, nc, [], []), 0, 0, BR.thresholds(0, L), 0
    k, cand, _ = BR.keys(flat, W, H, D, L)
    ks = np.sort(k[cand])[::-1]
    T = BR.select(ks, K)
    keep = cand & (k > T)
    out, kept = _emit(W, H, D, nc, flat, keep)
    return out, kept, T, BR.thresholds(T, L), int((cand & (k == T)).sum())


def thin_thresh(pay, th):
    """th: L floats (more are ignored) -> (bytes, kept)."""
    W, H, D, L, nc, flat = dense(pay)
    if flat.size == 0:
        return O.serialize(W, H, D, nc, [], []), 0
    t = np.asarray(th, np.float32)[:L]
    assert t.size == L and not np.isnan(t).any() and (t >= 0).all()
    lvl = LT.level_map(W, H, D, L).reshape(-1)
    with np.errstate(invalid="ignore"):
        keep = np.abs(flat) > t[lvl - 1]  # strict: False for NaN
    return _emit(W, H, D, nc, flat, keep)


def budgets(pay, rng=None):
    """{class: K} of the classes this payload can show: 0, 1, kept - 1, kept, kept + 1 (kept = its
    candidates), a tie class (T's key occurs more than once straddling K) and a uniform rank."""
    ks = sorted_keys(pay)
    c = len(ks)
    out = {"zero": 0, "one": 1, "all": c, "over": c + 1}
    if c >= 1:
        out["all_but_one"] = c - 1
    if c >= 2:
        eq = np.nonzero(ks[:-1] == ks[1:])[0]
        if eq.size:
            out["tie"] = int(eq[eq.size // 2]) + 1
        rng = rng or np.random.default_rng(c)
        out["rank"] = int(rng.integers(1, c))
    return out
