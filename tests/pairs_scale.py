"""Shared by test_pairs_scale_cpu.py and test_gpu_pairs_scale.py: the large batch
of the pair pipeline (wc_thin_*, wc_split_*, wc_merge), built once per process and
left unchanged.  TEST INFRASTRUCTURE ONLY.

The units of test_gpu_thin / test_gpu_layers have at most 5 pair tiles (one has
32).  Here every box is the smallest that crosses a limit of the code:

  (64, 64, 65)  65 tiles  one past WC_OPT_TOL_SOLO_TILES = 64; odd, L = 1
  (64, 64, 72)  72 tiles  L = 3: nine whole chunks of 8 tiles
  (64, 64, 68)  68 tiles  L = 2: eight whole chunks and one of 4
  (80, 64, 64)  80 tiles  L = 4
  (64, 64, 64)  64 tiles  L = 4: the solo limit itself

so a unit's select is split over workgroups with chunk = 8, lookback_sum's window
of 64 predecessor tiles slides, and both counts of a split exceed 2^16.

Payloads to thin and split: the thresh = 0 payload of a tol_rule.field box per
box above; a 65-tile unit with a pair at every position whose value bits are
log-uniform over every exponent, with +-0, NaN, +-inf, subnormals and 5000 equal
magnitudes; sparse units on the 80-tile box with 8 * 4096 - 1, 8 * 4096,
8 * 4096 + 1 and 9 * 4096 + 1 pairs (whole work items past the payload's pairs, the
pair count at a chunk boundary +-1); 0 and 1 pairs on the 72-tile box; N + 4097
pairs on the 68-tile box; and two 16^3 units that show the classes "inf" and
"last_zero".  Budgets: one K per class of budget_rule.classes() and K = c // 2 and
100, spread over CALLS calls of the whole batch.  Thresholds: per level a magnitude
that occurs there, 0.0, and +inf on one level.

Pairs to merge: see _merge_pairs()."""
import numpy as np

import budget_rule as BR
import decode_payloads as DP
import layers_rule as LR
import levels_ref as R
import modes_batches as MB
import pack_rule as PR
import thin_rule as TR
from tol_rule import field

TILE = 4096
SOLO = 64  # WC_OPT_TOL_SOLO_TILES' default
MAX_LEVELS = 4
BOX65, BOX72, BOX68, BOX80, BOX64 = (64, 64, 65), (64, 64, 72), (64, 64, 68), (80, 64, 64), (64, 64, 64)
FIELDS = [(BOX65, 1, 1), (BOX72, 3, 0), (BOX68, 2, 2), (BOX80, 4, 1), (BOX64, 4, 0)]  # (dims, L, field kind)
SPARSE = [(8 * TILE - 1, 4), (8 * TILE, 1), (8 * TILE + 1, 2), (9 * TILE + 1, 3)]     # (pairs, L) on BOX80
SPECIALS = np.array([0, 0x80000000, 0x7FC00000, 0xFF800001, 0x7F800000, 0xFF800000, 1, 0x80000003], np.uint32)
TIE = 5000
EXTRA = ("half", "hundred")  # beside budget_rule.CLASSES
_memo = {}


def cells(dims):
    return dims[0] * dims[1] * dims[2]


def plan_tiles(dims):
    return -(-cells(dims) // TILE)


def log_bits(rng, n, specials=True):
    """n value bit patterns: either sign, the exponent field uniform over 0..254 (subnormals included), a
    uniform mantissa; eight of them the specials."""
    bits = (rng.integers(0, 2, n, dtype=np.uint64) << 31 | rng.integers(0, 255, n, dtype=np.uint64) << 23 |
            rng.integers(0, 1 << 23, n, dtype=np.uint64)).astype(np.uint32)
    if specials and n >= 16:
        bits[rng.choice(n, SPECIALS.size, replace=False)] = SPECIALS
    return bits


class Unit:
    def __init__(self, name, dims, L, payload, kind):
        self.name, self.dims, self.L, self.payload, self.kind = name, dims, L, payload, kind
        self.pairs = (len(payload) - 20) // 8
        self.N = cells(dims)
        self.tiles = plan_tiles(dims)


def _at(rng, N, n):
    pos = np.sort(rng.choice(N, n, replace=False)) if n else np.zeros(0, np.int64)
    return (np.diff(pos, prepend=-1) - 1).astype(np.uint32)


def field_box(i):
    """The float32 box [D, H, W] behind field unit i."""
    dims, _, kind = FIELDS[i]
    return field(kind, *dims, seed=140 + i).astype(np.float32)


def _units():
    rng = np.random.default_rng(9500)
    out = []
    for i, (dims, L, _) in enumerate(FIELDS):
        out.append(Unit(f"field-{plan_tiles(dims)}", dims, L, R.payload(field_box(i), L, thresh=0.0)[0], "field"))
    N = cells(BOX65)
    bits = log_bits(rng, N)
    free = np.nonzero(~np.isin(bits, SPECIALS))[0]
    tie = rng.choice(free, TIE, replace=False)
    bits[tie] = (bits[tie] & np.uint32(0x80000000)) | np.float32(3.25).view(np.uint32)
    out.append(Unit("every-position", BOX65, 1, PR.standard(*BOX65, 1, np.zeros(N, np.uint32), bits), "crafted"))
    for n, L in SPARSE:
        pay = PR.standard(*BOX80, L, _at(rng, cells(BOX80), n), log_bits(rng, n))
        out.append(Unit(f"sparse-{n}", BOX80, L, pay, "sparse"))
    out.append(Unit("n=0", BOX72, 3, PR.standard(*BOX72, 3, np.zeros(0, np.uint32), np.zeros(0, np.uint32)), "few"))
    one = np.float32(-2.5).view(np.uint32).reshape(1)
    out.append(Unit("n=1", BOX72, 2, PR.standard(*BOX72, 2, np.array([200000], np.uint32), one), "few"))
    n = cells(BOX68) + TILE + 1  # a tile and one pair past N
    out.append(Unit("surplus", BOX68, 2, PR.standard(*BOX68, 2, np.zeros(n, np.uint32), log_bits(rng, n)), "surplus"))
    # the select's two classes that need special values, at 16^3 (budget_rule.SPEC's "tiny" and a special box)
    tiny = (rng.standard_normal((16, 16, 16)) * 1e-38).astype(np.float32)
    out.append(Unit("tiny", (16, 16, 16), 2, R.payload(tiny, 2, thresh=0.0)[0], "small"))
    inf = MB.special_box("minus_inf", (16, 16, 16), rng).astype(np.float32)
    out.append(Unit("inf", (16, 16, 16), 2, R.payload(inf, 2, thresh=0.0)[0], "small"))
    return out


def budgets(pay):
    """{class: K}: budget_rule.classes() on the keys of A(P), K = c // 2 and K = 100."""
    W, H, D, L, _, flat = TR.dense(pay)
    if flat.size == 0:
        ks = lv = np.zeros(0, np.int64)
    else:
        ks, lv = BR.sorted_keys(flat, W, H, D, L)
    out = BR.classes(ks, lv, L)
    out["half"] = len(ks) // 2
    out["hundred"] = 100
    return out


def level_mags(pay):
    """Per level 1..L: the sorted magnitudes (float32) of the candidates of A(P) there."""
    W, H, D, L, _, flat = TR.dense(pay)
    if flat.size == 0:
        return [np.zeros(0, np.float32)] * L
    _, cand, lvl = BR.keys(flat, W, H, D, L)
    return [np.sort(np.abs(flat[cand & (lvl == l)])) for l in range(1, L + 1)]


class View:
    """One call on the batch, in the shape test_gpu_thin.Dev and test_gpu_layers.SplitDev read:
    want[i] = thin_rule's tuple; split[i] = layers_rule's."""

    def __init__(self, S, K, thresh, want, split):
        self.us, self.n, self.dims, self.levels, self.units = S.us, S.n, S.dims, S.levels, S.units
        self.buf, self.off, self.extent = S.buf, S.off, S.extent
        self.K, self.thresh, self.want, self.split = K, thresh, want, split
        self.cap = [min(k, u.N) for u, k in zip(S.us, K)]

    def slots(self, budget):
        o, out = 4, []
        for i, u in enumerate(self.us):
            out.append(o)
            o += 24 + 8 * (self.cap[i] if budget else u.N)
        return out, o


class Scale:
    def __init__(self, capi):
        rng = np.random.default_rng(9501)
        self.us = _units()
        self.n = len(self.us)
        self.dims = [u.dims for u in self.us]
        self.levels = [u.L for u in self.us]
        self.units, _, self.extent = capi.make_units(self.dims)
        self.buf, self.off = DP.payload_layout([u.payload for u in self.us], rng)
        self.avail = [budgets(u.payload) for u in self.us]
        order = BR.CLASSES + EXTRA
        self.own = [[c for c in order if c in a] for a in self.avail]
        self.calls = max(len(o) for o in self.own)
        # call j: unit i at its class (i + j) mod its count, so a call mixes the classes
        self.shown = [[o[(i + j) % len(o)] for i, o in enumerate(self.own)] for j in range(self.calls)]
        self.budget = []
        for j in range(self.calls):
            K = [self.avail[i][c] for i, c in enumerate(self.shown[j])]
            split = [LR.split_budget(u.payload, k) for u, k in zip(self.us, K)]
            want = [(s[0], s[2], s[4], s[5], None) for s in split]
            th = np.zeros((self.n, MAX_LEVELS), np.float32)
            self.budget.append(View(self, K, th, want, split))
        # thresholds: an occurring magnitude per level; 0.0; the first with +inf on one level
        mags = [level_mags(u.payload) for u in self.us]
        occ = np.zeros((self.n, MAX_LEVELS), np.float32)
        for i, m in enumerate(mags):
            for l, a in enumerate(m):
                occ[i, l] = a[a.size // 2] if a.size else 0.0
        inf = occ.copy()
        for i, u in enumerate(self.us):
            inf[i, i % u.L] = np.inf
        self.thresh = []
        for th in (occ, np.zeros_like(occ), inf):
            split = [LR.split_thresh(u.payload, th[i, :u.L]) for i, u in enumerate(self.us)]
            want = [(s[0], s[2], 0, [], None) for s in split]
            self.thresh.append(View(self, [0xFFFFFFFF] * self.n, th, want, split))
        self.occurring = mags

    def where(self, cl):
        """[(call, unit)] that show class cl."""
        return [(j, i) for j in range(self.calls) for i in range(self.n) if self.shown[j][i] == cl]


def scale(wc):
    if "scale" not in _memo:
        _memo["scale"] = Scale(wc.capi)
    return _memo["scale"]


# ---- merge ---------------------------------------------------------------------------------------------------
def _merge_pairs():
    """a. alternating positions on the 72-tile box; b. a = every 71st position (two tiles that span the box), b all
    others; c. a = [0, 200 000), b the rest; d. blocks of 4097 positions in turn; e. a random 1 : 3 partition of
    every position of the 65-tile box; f. a random partition of the 68-tile box with 5000 and 70 pairs past N;
    g. case a with one side empty."""
    from test_gpu_layers import Pair
    rng = np.random.default_rng(9502)
    N72, N80, N68, N65 = cells(BOX72), cells(BOX80), cells(BOX68), cells(BOX65)
    every = np.arange(N72)
    out = [Pair("a:alternating", BOX72, 3, every[0::2], every[1::2], rng)]
    mine = every % 71 == 0
    out.append(Pair("b:every-71st", BOX72, 2, every[mine], every[~mine], rng))
    out.append(Pair("c:a-before-b", BOX80, 4, np.arange(200000), np.arange(200000, N80), rng))
    blocks = (np.arange(N68) // (TILE + 1)) % 2 == 0
    out.append(Pair("d:blocks-4097", BOX68, 2, np.arange(N68)[blocks], np.arange(N68)[~blocks], rng))
    quarter = rng.random(N65) < 0.25
    out.append(Pair("e:one-to-three", BOX65, 1, np.arange(N65)[quarter], np.arange(N65)[~quarter], rng))
    coin = rng.random(N68) < 0.5
    out.append(Pair("f:past-N", BOX68, 1, np.arange(N68)[coin], np.arange(N68)[~coin], rng, past=(5000, 70)))
    out.append(Pair("g:b-empty", BOX72, 1, every[0::2], [], rng))
    return out


def merge_case(wc):
    if "merge" not in _memo:
        from test_gpu_layers import MergeCase
        _memo["merge"] = MergeCase(wc, _merge_pairs(), 9503)
    return _memo["merge"]


def overlaps(M):
    """The batch with one position on both sides of two units: case a with b's last pair moved onto a's last
    position (the last live pair of either side, in the box's tile 71), case c with position 200 000 appended to a.
    -> (a buffer, a offsets, b buffer, b offsets, the two indices, a's payloads, b's payloads)."""
    by = {p.name: i for i, p in enumerate(M.ps)}
    apays, bpays = [p.pay[0] for p in M.ps], [p.pay[1] for p in M.ps]
    ia, ic = by["a:alternating"], by["c:a-before-b"]
    W, H, D, nc, apos, _ = LR.live_pairs(apays[ia])
    _, _, _, _, bpos, bbits = LR.live_pairs(bpays[ia])
    bpos = bpos.copy()
    assert bpos[-1] == W * H * D - 1 and apos[-1] == bpos[-1] - 1 and apos[-1] // TILE == 71
    bpos[-1] = apos[-1]
    bpays[ia] = LR.emit(W, H, D, nc, bpos, bbits)
    W, H, D, nc, apos, abits = LR.live_pairs(apays[ic])
    assert apos[-1] == 199999 and LR.live_pairs(bpays[ic])[4][0] == 200000
    apos = np.append(apos, 200000)
    apays[ic] = LR.emit(W, H, D, nc, apos, np.resize(abits, apos.size))
    rng = np.random.default_rng(9504)
    abuf, aoff = DP.payload_layout(apays, rng)
    bbuf, boff = DP.payload_layout(bpays, rng)
    return abuf, aoff, bbuf, boff, (ia, ic), apays, bpays
