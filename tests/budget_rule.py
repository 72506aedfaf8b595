"""Shared by the tests of the size-budget mode (test_budget_cpu.py,
test_gpu_budget.py, test_gpu_budget_fuzz.py, test_gpu_budget_mirror.py): the
numpy restatement of the rule include/wavelet_amd.h documents for
wc_budget_select / wc_forward_levels_budget, and the mixed batch of the GPU test
with its budgets, picked by rank from the sorted keys.  TEST INFRASTRUCTURE ONLY.

Only integers enter the rule: keys are int64 here so that nothing wraps."""
import numpy as np

import leveltol_rule as LT
import levels_ref as R
import modes_batches as M
from oracle import oracle as O
from tol_rule import HIST_SHIFT, f32_from_bits, field

LTOL_SHIFT = LT.LTOL_SHIFT
INF_BITS = 0x7F800000
MAX_LEVELS = 4


def level_step(l):
    """The key offset of level l (1-based)."""
    return (LTOL_SHIFT * (l - 1)) << HIST_SHIFT


def keys(flat, W, H, D, L):
    """-> (key int64 [N], candidate bool [N], level int64 [N]) of the final flat array."""
    m = (np.ascontiguousarray(flat, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64)
    lvl = LT.level_map(W, H, D, L).reshape(-1)
    cand = (m >= 1) & (m <= INF_BITS)
    return m + ((LTOL_SHIFT * (lvl - 1)) << HIST_SHIFT), cand, lvl


def sorted_keys(flat, W, H, D, L):
    """The candidates' (keys, levels) in descending key order (stable: flat order among equals)."""
    k, cand, lvl = keys(flat, W, H, D, L)
    k, lvl = k[cand], lvl[cand]
    order = np.argsort(-k, kind="stable")
    return k[order], lvl[order]


def select(ks, K):
    """T of the budget K on the descending candidate keys ks."""
    return 0 if len(ks) <= K else int(ks[K])


def thresholds(T, L):
    """thresh_1..L as Python floats."""
    out = []
    for l in range(1, L + 1):
        d = T - level_step(l)
        out.append(f32_from_bits(0 if d <= 0 else INF_BITS if d >= INF_BITS else d))
    return out


def prepare(box, L):
    """What every budget of one unit shares: (W, H, D, L, flat, keys, candidate mask, descending keys, their levels)."""
    b = np.ascontiguousarray(box, np.float32)
    D, H, W = b.shape
    if b.size == 0:
        z = np.zeros(0, np.int64)
        return W, H, D, L, np.zeros(0, np.float32), z, np.zeros(0, bool), z, z
    flat = R.decompose(b, L)
    k, cand, _ = keys(flat, W, H, D, L)
    ks, lv = sorted_keys(flat, W, H, D, L)
    return W, H, D, L, flat, k, cand, ks, lv


def payload_of(prep, K):
    """-> (payload bytes, kept, T, [thresh_l], ties) of budget K on a prepare()d unit:
    the pairs of exactly the candidates with key > T, in flat order."""
    W, H, D, L, flat, k, cand, ks, _ = prep
    nc = W * H * D if L == 1 else -L
    T = select(ks, K)
    th = thresholds(T, L)
    if flat.size == 0:
        return O.serialize(W, H, D, 0 if L == 1 else -L, [], []), 0, T, th, 0
    keep = cand & (k > T)
    m = np.where(keep, flat, np.float32(0.0)).astype(np.float32)
    runs, vals = O.threshold_rle(m, 0.0)
    assert len(runs) == int(keep.sum())
    return O.serialize(W, H, D, nc, runs, vals), len(runs), T, th, int((cand & (k == T)).sum())


def payload(box, L, K):
    """-> (payload bytes, kept, T, [thresh_l], ties).  Mirrors leveltol_rule.payload."""
    return payload_of(prepare(box, L), K)


# ---- the budgets of the GPU test, by rank ------------------------------------------------------------------
CLASSES = ("zero", "all", "over", "all_but_one", "tie", "low_00", "low_7f", "mid_000", "mid_fff", "top_differs",
           "mid_differs", "cross_level", "last_zero", "inf")


def classes(ks, lv, L):
    """{class: K} of the classes this unit can show.  ks, lv: sorted_keys().  With T = ks[K] (K < c):
    tie          ks[K-1] == ks[K]: the ties straddle the budget, kept < K
    low_00/7f    the low 7 bits of T; mid_000/fff: its middle 12 bits
    top_differs  ks[K-1] and ks[K] differ in the top digit (key >> 19)
    mid_differs  the same top digit, another middle digit
    cross_level  the same top digit, different keys, from different levels
    last_zero    0 < T <= level L's offset: thresh_L = 0.0f while thresh_1 > 0 (L >= 2)
    inf          T >= 0x7F800000: thresh_1 = +inf"""
    c = len(ks)
    out = {"zero": 0, "all": c, "over": c + 7}
    if c >= 1:
        out["all_but_one"] = c - 1
    if c < 2:
        return out

    def first(mask, lo=0):
        idx = np.nonzero(mask)[0]
        return None if idx.size == 0 else int(idx[idx.size // 2]) + lo

    top, mid = ks >> HIST_SHIFT, (ks >> 7) & 0xFFF
    cand = {
        "tie": first(ks[:-1] == ks[1:], 1),
        "low_00": first((ks & 0x7F) == 0),
        "low_7f": first((ks & 0x7F) == 0x7F),
        "mid_000": first(mid == 0),
        "mid_fff": first(mid == 0xFFF),
        "top_differs": first(top[:-1] != top[1:], 1),
        "mid_differs": first((top[:-1] == top[1:]) & (mid[:-1] != mid[1:]), 1),
        "cross_level": first((top[:-1] == top[1:]) & (ks[:-1] != ks[1:]) & (lv[:-1] != lv[1:]), 1) if L >= 2 else None,
        "last_zero": first(ks <= level_step(L)) if L >= 2 else None,
        "inf": first(ks >= INF_BITS),
    }
    out.update({k: v for k, v in cand.items() if v is not None})
    return out


# (dims, L, what): what = a tol_rule.field kind, or a tag.  The batch of test_gpu_leveltol.py's shapes, and a
# unit of tiny values (Gaussian x 1e-38: level-1 keys below level 2's offset, the "last_zero" class).
SPEC = [((4, 4, 4), 2, 0), ((8, 8, 8), 3, 1), ((16, 16, 16), 4, 2), ((12, 20, 8), 2, 0), ((48, 16, 80), 4, 0),
        ((64, 64, 64), 3, 2), ((64, 64, 72), 3, 0), ((16, 16, 24), 1, 0), ((4, 2, 6), 1, 1), ((0, 8, 8), 2, "empty"),
        ((16, 16, 16), 3, 3), ((8, 8, 8), 2, "tiny")] + [(d, L, t) for t, d, L in M.SPECIALS]
ONE_LEVEL = 7  # an L = 1 unit: its payloads decode through plain wc_inverse
CALLS = 6


class Batch:
    """The batch in one cell type with its reference results for CALLS calls, computed once and left
    unchanged.  want[j][i] = (payload, kept, T, [thresh_l], ties) of unit i in call j; budgets[j][i] its K;
    shown[j][i] the class that K was picked for."""

    def __init__(self, capi, dtype, seed=8300):
        rng = np.random.default_rng(seed)
        self.dtype = dtype
        self.dims = [d for d, _, _ in SPEC]
        self.levels = [L for _, L, _ in SPEC]
        self.n = len(SPEC)
        self.units, _, self.extent = capi.make_units(self.dims)
        self.cells = np.zeros(self.extent, dtype)
        self.boxes, self.prep = [], []
        for i, ((W, H, D), L, what) in enumerate(SPEC):
            if what == "empty":
                b = np.zeros((D, H, W), np.float64)
            elif what == "tiny":
                b = rng.standard_normal((D, H, W)) * 1e-38
            elif isinstance(what, str):
                b = M.special_box(what, (W, H, D), rng)
            else:
                b = field(what, W, H, D, seed=60 + i).astype(np.float64)
            o = self.units[i].cell_offset
            self.cells[o:o + b.size] = b.ravel().astype(dtype)
            b32 = M.narrow(O, b, dtype)
            self.boxes.append(b32)
            self.prep.append(prepare(b32, L))
        self.avail = [classes(p[7], p[8], p[3]) for p in self.prep]
        self.shown = self._assign()
        self.budgets = [[self.avail[i][self.shown[j][i]] for i in range(self.n)] for j in range(CALLS)]
        self.want = [[payload_of(self.prep[i], self.budgets[j][i]) for i in range(self.n)] for j in range(CALLS)]
        self.regen = [[R.decode(w[0])[0] for w in row] for row in self.want]
        self.owned = np.zeros(self.extent, bool)
        for i, b in enumerate(self.boxes):
            o = self.units[i].cell_offset
            self.owned[o:o + b.size] = True

    def _assign(self):
        """shown[j][i]: every class that some unit can show gets a slot (the rarest classes first, each at
        the unit with the fewest classes still to place); the free slots rotate through the unit's own classes."""
        slots = [[None] * self.n for _ in range(CALLS)]
        free = [CALLS] * self.n
        for cl in sorted(CLASSES, key=lambda c: sum(c in a for a in self.avail)):
            have = [i for i in range(self.n) if cl in self.avail[i] and free[i]]
            if not have:
                continue
            i = max(have, key=lambda u: (free[u], -u))  # the unit with the most room, the first of those
            slots[CALLS - free[i]][i] = cl
            free[i] -= 1
        for i in range(self.n):
            own = [c for c in CLASSES if c in self.avail[i]]
            for j in range(CALLS):
                if slots[j][i] is None:
                    slots[j][i] = own[(i + 3 * j) % len(own)]
        return slots
