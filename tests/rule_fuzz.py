"""Seeded cases for the rule-driven modes of the multi-level transform: the pointwise
error bound (wc_forward_levels_maxerr) and the per-level RMSE tolerance
(wc_forward_levels_tol).  TEST INFRASTRUCTURE ONLY: shared by
tests/test_rule_fuzz_cpu.py, which runs the cases through the host rules and proves
that they hold what the GPU tests rely on, and tests/test_gpu_maxerr_fuzz.py /
tests/test_gpu_leveltol_fuzz.py, which run them on the device.  Every expected result
is a restatement's (maxerr_rule.py, leveltol_rule.py, levels_ref.py), computed once per
case, memoised and left unchanged.

The batches are modes_batches.levels_batch's without the units these modes refuse
(cells and an odd dimension), as test_gpu_budget_fuzz.FuzzCase filters them, at the
batch's own cell offsets: random gaps, every third unit at an odd element offset."""
import math

import numpy as np

import leveltol_rule as LT
import levels_ref as R
import maxerr_rule as MR
import maxerr_tiles as MT
import modes_batches as M

_memo = {}


class Batch:
    """units, n, extent, cells (the caller's dtype), owned (bool per cell), dims, levels, x (each unit's cells
    [D, H, W] in the caller's dtype), boxes (as the transform sees them, float32)."""

    def __init__(self, capi, dtype, dims, levels, xs, boxes, offsets=None, align=4):
        self.dtype, self.dims, self.levels, self.x, self.boxes = dtype, list(dims), list(levels), list(xs), list(boxes)
        self.n = len(self.dims)
        self.units, _, self.extent = capi.make_units(self.dims, offsets, align=align)
        self.cells = np.zeros(max(self.extent, 1), dtype)
        self.owned = np.zeros(self.cells.size, bool)
        for i, x in enumerate(self.x):
            o = self.units[i].cell_offset
            assert not self.owned[o:o + x.size].any()
            self.cells[o:o + x.size] = x.ravel()
            self.owned[o:o + x.size] = True


def _levels_units(capi, oracle, seed):
    LB = M.levels_batch(oracle, seed)
    keep = [i for i, d in enumerate(LB.dims) if not (d[0] * d[1] * d[2] and (d[0] | d[1] | d[2]) & 1)]
    assert all(keep[u] == u for u in range(len(M.PINNED) + len(M.SPECIALS)))
    B = Batch(capi, LB.dtype, [LB.dims[i] for i in keep], [LB.levels[i] for i in keep],
              [LB.boxes[i].astype(LB.dtype) for i in keep], [M.narrow(oracle, LB.boxes[i], LB.dtype) for i in keep],
              [LB.offsets[i] for i in keep], align=1)
    B.seed = seed
    return B


def finite_max(x):
    """max |x| over the finite cells, in double; 1.0 without any."""
    f = np.abs(np.asarray(x, np.float64))
    f = f[np.isfinite(f)]
    return float(f.max()) if f.size else 1.0


def maxerr_case(capi, oracle, seed):
    """The levels batch of `seed` with a bound per unit, drawn from default_rng(9300 + seed): a kind in 0..7, an
    exponent and a bin b for every unit, whichever the kind uses, so that a unit's draw does not move the next
    one's.  Kind 0: E = 0.0; 1: +inf; 2..5: 10^U(-5, 0.3) x the unit's max |x| over its finite cells; 6: E =
    err(b) of the restatement at the bin b in 1..4095; 7: the double just below it.  Kinds 6 and 7 fall back to
    kind 2 where err(b) is 0 or not finite.  A unit of kind 6 or 7 also carries the twin decision, the
    restatement's b* under the other bound of the two: twin[i] = (E', b*'), None elsewhere.  The batch itself
    holds one bound per unit; the twin is for the CPU leg, which shows that the pair of bounds moves b*.
    Adds E, kind, twin, flat (the final arrays) and want[i] = maxerr_rule.payload(x, L, E, narrowed)."""
    key = ("maxerr", seed)
    if key in _memo:
        return _memo[key]
    B = _levels_units(capi, oracle, seed)
    rng = np.random.default_rng(9300 + seed)
    B.E, B.kind, B.twin, B.flat, B.want = [], [], [], [], []
    for i in range(B.n):
        x, L = B.x[i], B.levels[i]
        kind, ex, b = int(rng.integers(0, 8)), float(rng.uniform(-5.0, 0.3)), int(rng.integers(1, 4096))
        flat = R.decompose(B.boxes[i], L) if x.size else np.zeros(0, np.float32)
        twin = None
        if kind >= 6:
            U = MR.Unit(x, flat, L)
            e = U.err(b) if x.size else 0.0
            if math.isfinite(e) and e > 0.0:
                below = float(np.nextafter(e, 0.0))
                E, other = (e, below) if kind == 6 else (below, e)
                twin = (other, MR.search(U, other))
            else:
                kind = 2
        if kind == 0:
            E = 0.0
        elif kind == 1:
            E = math.inf
        elif kind < 6:
            E = 10.0 ** ex * finite_max(x)
        B.E.append(E)
        B.kind.append(kind)
        B.twin.append(twin)
        B.flat.append(flat)
        B.want.append(MR.payload(x, L, E, narrowed=B.boxes[i]))
    _memo[key] = B
    return B


def leveltol_case(capi, oracle, seed):
    """The levels batch of `seed` with a tolerance per unit in modes_batches.tol_batch's draw, from a
    default_rng(9300 + seed) of its own: a kind in 0..5; 0 gives 0.0, 1 gives +inf, otherwise 10^U(-6, 3) x the
    RMS of the unit's finite narrowed cells.  Kind and exponent are drawn for every unit, as in maxerr_case.
    Adds tol, flat, want[i] = (payload, kept, [thresh_l], bound), stop (the walk's (s*, l*) or None), regen."""
    key = ("leveltol", seed)
    if key in _memo:
        return _memo[key]
    B = _levels_units(capi, oracle, seed)
    rng = np.random.default_rng(9300 + seed)
    B.tol, B.flat, B.want, B.stop, B.regen = [], [], [], [], []
    for i in range(B.n):
        b32, L = B.boxes[i], B.levels[i]
        W, H, D = B.dims[i]
        f = b32.astype(np.float64)
        f = f[np.isfinite(f)]
        rms = float(np.sqrt(np.mean(f * f))) if f.size else 0.0
        k, ex = int(rng.integers(0, 6)), float(rng.uniform(-6.0, 3.0))
        tol = 0.0 if k == 0 else math.inf if k == 1 else 10.0 ** ex * rms
        pay, kept, th, bd, flat, _ = LT.payload(b32, L, tol)
        counts = LT.level_counts(flat, W, H, D, L) if flat.size else np.zeros((L, LT.HIST_BINS), np.uint64)
        B.tol.append(tol)
        B.flat.append(flat)
        B.want.append((pay, kept, th, bd))
        B.stop.append(LT.pick(counts, L, flat.size, tol)[2])
        B.regen.append(R.decode(pay)[0])
    _memo[key] = B
    return B


def _tile_want(oracle, u, dtype):
    key = ("tile", u.name, u.tile, dtype)
    if key not in _memo:
        x = u.box.astype(np.float64) * (1.0 + 2.0 ** -30) if dtype == np.float64 else u.box  # differs from its narrowing
        b32 = M.narrow(oracle, x, dtype)
        E = 1e-2 * finite_max(x)
        _memo[key] = (x, b32, E, MR.payload(x, u.L, E, narrowed=b32))
    return _memo[key]


def tiles_case(capi, oracle, maxl, dtype, odd):
    """The units of maxerr_tiles.units() of at most maxl levels, their target tiles in the geometry of a call
    whose largest L is maxl, E = 1e-2 x max |x|; packed at make_units' default alignment, or with every unit at
    an odd element offset.  Adds us, E, want as maxerr_case."""
    key = ("tiles", maxl, dtype, odd)
    if key in _memo:
        return _memo[key]
    us = [u for u in MT.units(MT.ty_of(maxl)) if u.L <= maxl]
    assert max(u.L for u in us) == maxl
    got = [_tile_want(oracle, u, dtype) for u in us]
    offsets, cur = None, 0
    if odd:
        offsets = []
        for u in us:
            cur += 1 - cur % 2 + 2 * (len(offsets) % 3)
            offsets.append(cur)
            cur += u.box.size
    B = Batch(capi, dtype, [u.dims for u in us], [u.L for u in us], [g[0] for g in got], [g[1] for g in got], offsets)
    B.us, B.E, B.want = us, [g[2] for g in got], [g[3] for g in got]
    assert not odd or all(B.units[i].cell_offset % 2 for i in range(B.n))
    _memo[key] = B
    return B
