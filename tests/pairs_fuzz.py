"""Seeded random batches for the pair pipeline (wc_thin_*, wc_split_*, wc_merge).
TEST INFRASTRUCTURE ONLY: shared by tests/test_pairs_scale_cpu.py, which runs the
batches through the host rule, and tests/test_gpu_pairs_fuzz.py, which runs them
on the device; tol_batch() adds a tolerance per unit for tests/test_rule_fuzz_cpu.py
and tests/test_gpu_pairs_tol_fuzz.py.  Every expected result is the numpy
restatement's (thin_rule.py, layers_rule.py, thin_tol_rule.py), computed here once
per seed.

A batch: about 24 units of at most 2^15 cells (the 2-adic shapes of modes_batches,
odd boxes at L = 1, a box without cells) and one of 65-70 pair tiles; L from what
the box admits; a pair count from {0, 1, 63..65, 4095..4097, uniform below 1.2 N};
heavy-tailed runs, in some units with a tail that overshoots N (never a negative
run); value bits log-uniform over every exponent, or quantised to 64 magnitudes
(ties), with the specials sprinkled in.  Per unit one K of thin_rule.budgets() and
budget_rule.classes(), thresholds from its own magnitudes and {0, +inf}, and its
live pairs dealt at random to two or three layers, some with pairs past N."""
import numpy as np

import budget_rule as BR
import layers_rule as LR
import levels_ref as R
import pack_rule as PR
import thin_rule as TR
from modes_batches import ES, MS
from pairs_scale import SPECIALS, TILE, cells, log_bits

COUNTS = (0, 1, 63, 64, 65, 4095, 4096, 4097)
SMALL = 1 << 15
M31 = 2 ** 31 - 1
_memo = {}


class Unit:
    """name, dims, L, N, pairs, payload; K, thresh [4]; split = layers_rule.split_budget(payload, K), tsplit =
    split_thresh(payload, thresh); K2, split2 = split_budget(rest, K2); canon; layers (three payloads, the third
    may be empty), merged01 = merge(layers[0], layers[1]), merged = all three."""


def _axis(rng, e0):
    while True:
        v = int(rng.choice(MS)) << int(min(ES - 1, e0 + rng.integers(0, 3)))
        if v <= 128:
            return v


def _dims(rng):
    if rng.random() < 0.2:
        return tuple(int(x) for x in rng.choice([1, 3, 5, 7, 9, 15, 31], size=3))
    while True:
        e0 = int(rng.integers(0, 4))
        d = tuple(_axis(rng, e0) for _ in range(3))
        if cells(d) <= SMALL:
            return d


def _runs(rng, N, n):
    """n runs: heavy-tailed shares of the free positions, so all pairs lie below N (n <= N); one unit in four
    stretches them so that a tail overshoots N, sometimes by one run of up to 2^31 - 1."""
    if n == 0:
        return np.zeros(0, np.uint32)
    if n > N:  # surplus: at most a few gaps
        runs = np.zeros(n, np.int64)
        runs[rng.integers(0, n, 3)] = rng.integers(0, 3, 3)
        return runs.astype(np.uint32)
    w = rng.pareto(1.2, n) + 1e-9
    over = rng.random() < 0.25
    stretch = rng.uniform(1.1, 3.0) if over else 1.0
    runs = np.floor(w / w.sum() * (N - n) * stretch).astype(np.int64)
    if over and rng.random() < 0.5:
        runs[int(rng.integers(0, n))] = int(rng.integers(N, M31 + 1))
    return np.minimum(runs, M31).astype(np.uint32)


def _bits(rng, n):
    mode = int(rng.integers(0, 3))
    bits = log_bits(rng, n, specials=False)
    if mode >= 1:  # 64 magnitudes: ties everywhere (mode 2: on half the pairs)
        mags = log_bits(rng, 64, specials=False) & np.uint32(0x7FFFFFFF)
        q = (bits & np.uint32(0x80000000)) | mags[rng.integers(0, 64, n)]
        bits = q if mode == 1 else np.where(rng.random(n) < 0.5, q, bits)
    pick = rng.random(n) < 0.03
    bits[pick] = SPECIALS[rng.integers(0, SPECIALS.size, int(pick.sum()))]
    return bits.astype(np.uint32)


def _layers(rng, u):
    """The live pairs of u dealt to two or three layers; a layer may get up to 70 pairs past N."""
    W, H, D, nc, pos, bits = LR.live_pairs(u.payload)
    p = rng.uniform(0.01, 0.99)
    three = rng.random() < 0.5
    side = (rng.random(pos.size) >= p).astype(np.int64)
    if three:
        side[(side == 1) & (rng.random(pos.size) < rng.uniform(0.01, 0.99))] = 2
    out = []
    for s in range(3):
        lp, lb = pos[side == s], bits[side == s]
        runs = (np.diff(lp, prepend=-1) - 1).astype(np.int64)
        if u.N and rng.random() < 0.3:  # pairs past N: the first exactly at N
            extra = int(rng.integers(1, 71))
            last = int(lp[-1]) if lp.size else -1
            runs = np.concatenate([runs, [u.N - last - 1], rng.integers(0, 3, extra - 1)])
            lb = np.concatenate([lb, log_bits(rng, extra, specials=False)])
        out.append(PR.standard(W, H, D, u.L, runs.astype(np.uint32), lb.astype(np.uint32)))
    return out


def _unit(rng, name, dims, count):
    u = Unit()
    u.name, u.dims, u.N = name, dims, cells(dims)
    u.L = int(rng.integers(1, R.levels_for(*dims, R.MAX_LEVELS) + 1))
    n = count if count >= 0 else int(rng.integers(0, int(1.2 * u.N) + 1))
    if u.N == 0:
        n = 0
    u.payload = PR.standard(*dims, u.L, _runs(rng, u.N, n), _bits(rng, n))
    u.pairs = n
    u.canon = LR.canon(u.payload)
    # K: one class of thin_rule.budgets() and budget_rule.classes()
    W, H, D, L, _, flat = TR.dense(u.payload)
    ks, lv = BR.sorted_keys(flat, W, H, D, L) if flat.size else (np.zeros(0, np.int64),) * 2
    pool = dict(BR.classes(ks, lv, L))
    pool.update({"thin:" + k: v for k, v in TR.budgets(u.payload, rng).items()})
    names = sorted(pool)
    u.cls = names[int(rng.integers(0, len(names)))]
    u.K = int(pool[u.cls])
    u.split = LR.split_budget(u.payload, u.K)
    # thresholds: the unit's own magnitudes, 0 and +inf
    cand = np.abs(flat[BR.keys(flat, W, H, D, L)[1]]) if flat.size else np.zeros(0, np.float32)
    u.thresh = np.zeros(R.MAX_LEVELS, np.float32)
    for l in range(u.L):
        c = rng.random()
        u.thresh[l] = 0.0 if c < 0.15 or cand.size == 0 else np.inf if c < 0.25 else cand[int(rng.integers(0, cand.size))]
    u.tsplit = LR.split_thresh(u.payload, u.thresh[:u.L])
    rp = u.split[3]
    u.K2 = int(rng.choice([0, rp // 2, rp, rp + 1, int(rng.integers(0, rp + 1))]))
    u.split2 = LR.split_budget(u.split[1], u.K2)
    u.layers = _layers(rng, u)
    u.merged01 = LR.merge(u.layers[0], u.layers[1])
    u.merged = LR.merge(u.merged01, u.layers[2])
    return u


def batch(seed):
    if seed in _memo:
        return _memo[seed]
    rng = np.random.default_rng(17000 + seed)

    class B:
        pass

    n = int(rng.integers(22, 27))
    dims = [_dims(rng) for _ in range(n - 2)]
    d = [int(rng.choice(MS)) * 2 for _ in range(3)]
    d[int(rng.integers(0, 3))] = 0
    dims.insert(int(rng.integers(0, len(dims) + 1)), tuple(d))
    big = [(64, 64, int(rng.integers(65, 71))), (int(rng.integers(65, 71)), 64, 64)][int(rng.integers(0, 2))]
    dims.insert(int(rng.integers(0, len(dims) + 1)), big)
    B.seed, B.n = seed, n
    deck = rng.permutation(list(COUNTS) + [-1] * len(COUNTS))  # every count of COUNTS once, as many uniform draws
    B.us = [_unit(rng, f"s{seed}u{i}", d, int(deck[i % deck.size])) for i, d in enumerate(dims)]
    B.dims = dims
    B.levels = [u.L for u in B.us]
    _memo[seed] = B
    return B


def tol_batch(seed):
    """The units of batch(seed) that wc_thin_tol / wc_split_tol take (thin_tol_rule.accepted), each with a
    tolerance from a default_rng(9400 + seed) of its own, so that batch(seed) stays as it was: a kind in 0..5; 0
    gives 0.0, 1 gives +inf, otherwise 10^U(-3, 0.5) x thin_tol_rule.weighted_rms(payload).  Every unit of
    batch(seed) gets the fields tol, thin_tol = thin_tol_rule.thin_tol(payload, tol) and split_tol =
    thin_tol_rule.split_tol(payload, tol); None on the refused ones.  -> us, n, dims, levels, tol, want, split."""
    import thin_tol_rule as TT
    if ("tol", seed) in _memo:
        return _memo[("tol", seed)]
    rng = np.random.default_rng(9400 + seed)

    class T:
        pass

    T.seed, T.us = seed, []
    for u in batch(seed).us:
        u.tol = u.thin_tol = u.split_tol = None
        if not TT.accepted(*u.dims, u.L):
            continue
        k, ex = int(rng.integers(0, 6)), float(rng.uniform(-3.0, 0.5))
        u.tol = 0.0 if k == 0 else float(np.inf) if k == 1 else 10.0 ** ex * TT.weighted_rms(u.payload)
        u.thin_tol = TT.thin_tol(u.payload, u.tol)
        u.split_tol = TT.split_tol(u.payload, u.tol)
        T.us.append(u)
    T.n = len(T.us)
    T.dims, T.levels = [u.dims for u in T.us], [u.L for u in T.us]
    T.tol = np.array([u.tol for u in T.us], np.float64)
    T.want, T.split = [u.thin_tol for u in T.us], [u.split_tol for u in T.us]
    _memo[("tol", seed)] = T
    return T
