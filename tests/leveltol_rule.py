"""Shared by the tests of the RMSE tolerance on the multi-level transform
(test_leveltol_cpu.py, test_gpu_leveltol.py): the numpy / Python-float
restatement of the rule include/wavelet_amd.h documents for
wc_tol_levels_threshold and wc_forward_levels_tol.  TEST INFRASTRUCTURE ONLY.

Python floats are IEEE doubles and every operation below is rounded on its
own, as the rule demands (no fused multiply-add)."""
import math

import numpy as np

import levels_ref as R
from oracle import oracle as O
from tol_rule import FLT_MAX, HIST_BINS, HIST_SHIFT, f32_from_bits

LTOL_SHIFT = 24


def level_map(W, H, D, L):
    """int array (W, H, D): the level 1..L of every coefficient of the final array."""
    lvl = np.ones((W, H, D), np.int64)
    for j in range(1, L):
        lvl[:W >> j, :H >> j, :D >> j] = j + 1
    return lvl


def level_counts(flat, W, H, D, L):
    """cnt[l - 1][b] (uint64 [L, HIST_BINS]) of the final flat array; NaN not counted."""
    bits = np.ascontiguousarray(flat, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    lvl = level_map(W, H, D, L).reshape(-1)
    cnt = np.zeros((L, HIST_BINS), np.uint64)
    ok = bits <= 0x7F800000
    for l in range(1, L + 1):
        sel = ok & (lvl == l)
        cnt[l - 1] = np.bincount((bits[sel] >> HIST_SHIFT).astype(np.int64), minlength=HIST_BINS)
    return cnt


def bin_threshold(bstar):
    if bstar == 0:
        return 0.0
    if bstar >= 0xFF0:
        return FLT_MAX
    return f32_from_bits((bstar << HIST_SHIFT) - 1)


def pick(counts, L, ncoeff, tol):
    """-> ([thresh_1 .. thresh_L] as Python floats, bound, (s*, l*) or None)."""
    cnt = np.asarray(counts).reshape(L, HIST_BINS)
    tol = float(tol)
    budget = (tol * tol) * float(ncoeff)
    # the visited pairs in lexicographic (s, l) order
    ls, bs = np.nonzero(cnt)
    order = sorted(zip((bs + LTOL_SHIFT * ls).tolist(), (ls + 1).tolist(), bs.tolist()))
    S, stop = 0.0, None
    for s, l, b in order:
        hi = f32_from_bits((b + 1) << HIST_SHIFT) if b < 0xFEF else math.inf
        t = S + float(int(cnt[l - 1, b])) * (float(8 ** l) * (hi * hi))
        if not (t <= budget):
            stop = (s, l)
            break
        S = t
    thresh = []
    for l in range(1, L + 1):
        bstar = HIST_BINS
        if stop is not None:
            bstar = min(max(stop[0] + (1 if l < stop[1] else 0) - LTOL_SHIFT * (l - 1), 0), HIST_BINS)
        thresh.append(bin_threshold(bstar))
    bound = math.sqrt(S / float(ncoeff)) if ncoeff else 0.0
    return thresh, bound, stop


def mask(flat, W, H, D, L, thresh):
    """The final array with every coefficient that fails |c| > thresh_lvl set to +0."""
    f = np.ascontiguousarray(flat, np.float32)
    t = np.asarray(thresh, np.float32)[level_map(W, H, D, L).reshape(-1) - 1]
    with np.errstate(invalid="ignore"):
        keep = np.abs(f) > t
    return np.where(keep, f, np.float32(0.0)).astype(np.float32)


def payload(box, L, tol):
    """-> (payload bytes, kept, [thresh_l], bound, final flat array, masked array)."""
    b = np.ascontiguousarray(box, np.float32)
    D, H, W = b.shape
    nc = W * H * D if L == 1 else -L
    if b.size == 0:
        th, bd, _ = pick(np.zeros((L, HIST_BINS), np.uint64), L, 0, tol)
        return O.serialize(W, H, D, 0 if L == 1 else -L, [], []), 0, th, bd, np.zeros(0, np.float32), np.zeros(0, np.float32)
    flat = R.decompose(b, L)
    th, bd, _ = pick(level_counts(flat, W, H, D, L), L, flat.size, tol)
    m = mask(flat, W, H, D, L, th)
    runs, vals = O.threshold_rle(m, 0.0)
    return O.serialize(W, H, D, nc, runs, vals), len(runs), th, bd, flat, m
