"""Crafted decoder inputs: valid payloads no encoder of a real field emits.
TEST INFRASTRUCTURE ONLY: the generator of tests/test_decode_payloads_cpu.py and
tests/test_gpu_decode_payloads.py; the product never imports it.

A decoder reads a header and nrle pairs {int32 run, uint32 value bits}.  Valid
here: the header is the unit's (ncoeff = W*H*D, or -L for L >= 2), nrle >= 0,
every run >= 0.  The rule the decoders follow for such a payload is the
project's own (wc_pairscan.h): pair k sits at p_k = (sum of run + 1 over pairs
<= k) - 1 in exact arithmetic, positions never decrease, and every pair at or
past ncoeff is dropped.  The reference's rle_decode keeps the position in an
int, so a run sum past 2^31 - 1 is undefined there; rule_decode() below is the
rule in Python ints, and the oracle's 64-bit wco_rle_decode agrees with it
(test_decode_payloads_cpu.py).

Every unit carries the class it was built for; classify() finds the classes
again from the runs (and the bits, for the value classes) alone.
"""
import functools
from typing import NamedTuple

import numpy as np

import pack_rule as PR
import region_ref as G

M = 2 ** 31 - 1          # the largest run
TILE = 4096              # pairs per decode tile (csrc/wc_internal.h kFlatTile, kRixTile)
TRAIL = 70               # run-0 pairs behind every overshoot: more than one round of a wave
MARK = 0x42F60000        # 123.0f: the value of those pairs

RIX = (32, 16, 32)       # four pair tiles; row-indexed inverse (even W and H, D % 8 == 0)
DENSE = [(32, 16, 34), (33, 17, 31)]  # dense decode, odd tail
CUBE = (32, 32, 32)      # levels 1..3; the coarse and region decoders
LONG = (2, 2, 2288)      # falls back from the row index at the default LDS budget
TINY = [(2, 2, 8), (3, 5, 7), (2, 2, 2), (1, 1, 1), (0, 4, 4)]
# (dims, L) of the boxes with pair tiles
BIG = [(RIX, 1), (DENSE[0], 1), (DENSE[1], 1), (CUBE, 1), (CUBE, 2), (CUBE, 3), (LONG, 1)]
SMALL = [(d, 1) for d in TINY]

FIXED_COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193)
REL_COUNTS = (-1, 0, 1, 5, 4096, 4097, 8193)
POSITION = ("pos:last", "pos:dropped", "pos:last+4097", "pos:row-starts", "pos:row-ends", "pos:sparse-rows",
            "pos:tile-then-jump", "pos:two-tiles-past")
OVERSHOOT = ("ov:first", "ov:one-round", "ov:two-rounds", "ov:two-waves", "ov:two-tiles", "ov:lookback", "ov:all-sat")
VALUES = ("val:random", "val:specials", "val:-0-blocks", "val:+0", "val:nan")
END = ("end:last", "end:tile-1", "end:tile", "end:tile+1")
NANS = np.array([0x7F800001, 0xFF800001, 0x7FC00000, 0xFFC00000, 0x7FBFFFFF, 0xFFFFFFFF], np.uint32)  # s, s, q, q, s, q
ALL_CLASSES = tuple(f"n={n}" for n in FIXED_COUNTS) + tuple(f"n=nc{d:+d}" for d in REL_COUNTS) + \
    POSITION + OVERSHOOT + VALUES + END + ("levels:2", "levels:3")


class Unit(NamedTuple):
    name: str
    cls: str       # the class it was built for
    dims: tuple    # (W, H, D)
    L: int
    runs: np.ndarray  # uint32, every run <= M
    bits: np.ndarray  # uint32

    @property
    def ncoeff(self):
        return self.dims[0] * self.dims[1] * self.dims[2]

    @property
    def payload(self):
        return PR.standard(*self.dims, self.L, self.runs, self.bits)


def rule_decode(runs, bits, ncoeff):
    """The project's rule in Python ints -> the flat array's bits."""
    out, idx = [0] * ncoeff, 0
    for run, b in zip(runs.tolist(), bits.tolist()):
        idx += run
        if idx >= ncoeff:
            break  # positions never decrease: every later pair is dropped too
        out[idx] = b
        idx += 1
    return np.array(out, np.uint32)


def positions(runs):
    """Exact positions (int64: at most 2^17 pairs of at most 2^31 each)."""
    return np.cumsum(np.asarray(runs, np.int64) + 1) - 1


def _finite_bits(rng, n):
    """n finite, non-zero, normal float32 bit patterns of either sign."""
    v = (rng.standard_normal(n) * 8.0 + np.where(rng.random(n) < 0.5, -40.0, 40.0)).astype(np.float32)
    return v.view(np.uint32).copy()


def _unit(name, cls, dims, L, runs, bits=None, rng=None):
    runs = np.asarray(runs, np.uint64)
    assert runs.size == 0 or int(runs.max()) <= M
    runs = runs.astype(np.uint32)
    if bits is None:
        bits = _finite_bits(rng or np.random.default_rng(runs.size), runs.size)
    bits = np.asarray(bits, np.uint32)
    assert bits.shape == runs.shape
    W, H, D = dims
    return Unit(f"{name}@{W}x{H}x{D}/L{L}", cls, tuple(dims), L, runs, bits)


def _from_positions(pos):
    pos = np.asarray(pos, np.int64)
    return np.diff(pos, prepend=-1) - 1


# ------------------------------------------------------------ pair counts --
def count_units(dims, L, rng):
    """All runs 0 (pair index = position): the fixed counts the box has cells
    for, and the counts around and past ncoeff."""
    nc = dims[0] * dims[1] * dims[2]
    seen, out = set(), []
    for cls, n in [(f"n={n}", n) for n in FIXED_COUNTS if n <= nc] + [(f"n=nc{d:+d}", nc + d) for d in REL_COUNTS]:
        if n < 0 or n in seen:
            continue
        seen.add(n)
        out.append(_unit(cls, cls, dims, L, np.zeros(n, np.uint32), rng=rng))
    return out


# -------------------------------------------------------------- positions --
def position_units(dims, L, rng):
    W, H, D = dims
    nc = W * H * D
    out = []
    if nc == 0:
        return out
    out.append(_unit("last", "pos:last", dims, L, [nc - 1], rng=rng))
    out.append(_unit("dropped", "pos:dropped", dims, L, [nc], rng=rng))
    out.append(_unit("last+4097", "pos:last+4097", dims, L, [nc - 1] + [0] * 4097, rng=rng))
    rows = np.arange(W * H, dtype=np.int64) * D
    out.append(_unit("row-starts", "pos:row-starts", dims, L, _from_positions(rows), rng=rng))
    out.append(_unit("row-ends", "pos:row-ends", dims, L, _from_positions(rows + D - 1), rng=rng))
    if nc > 7 * D + 3:  # a box of more than seven rows
        out.append(_unit("sparse-rows", "pos:sparse-rows", dims, L, _from_positions(np.arange(0, nc, 7 * D + 3)), rng=rng))
    if nc - D >= TILE:  # a full first tile, then one run to the start of the last row
        out.append(_unit("tile-then-jump", "pos:tile-then-jump", dims, L,
                         _from_positions(np.concatenate([np.arange(TILE), [nc - D, nc - D + 1]])), rng=rng))
    if nc >= 3 * TILE:  # tile 0 inside the box, the first pair of tile 1 jumps past it
        runs = np.zeros(3 * TILE, np.int64)
        runs[TILE] = nc
        runs[TILE + 1:] = rng.integers(0, 4, 2 * TILE - 1)
        out.append(_unit("two-tiles-past", "pos:two-tiles-past", dims, L, runs, rng=rng))
    return out


# -------------------------------------------------------------- overshoot --
def _close(runs, bits, nc, rng):
    """Append runs until the exact sum of run + 1, taken mod 2^32, is below
    ncoeff, then TRAIL run-0 pairs of MARK: a wrapping 32-bit sum puts them
    inside the box, the rule drops them."""
    runs = [int(r) for r in runs]
    S = sum(r + 1 for r in runs)
    assert S > nc  # the payload has left the box
    while S % 2 ** 32 >= max(nc, 1):
        f = 2 ** 32 - 1 - S % 2 ** 32  # brings the wrapped sum to 0
        f = f if f <= M else M
        runs.append(f)
        S += f + 1
    extra = len(runs) - len(bits)
    bits = np.concatenate([bits, _finite_bits(rng, extra), np.full(TRAIL, MARK, np.uint32)])
    return np.array(runs + [0] * TRAIL, np.uint64), bits


def overshoot_units(dims, L, rng):
    W, H, D = dims
    nc = W * H * D
    out = []

    def add(name, runs):
        runs = np.asarray(runs, np.int64)
        r, b = _close(runs, _finite_bits(rng, runs.size), nc, rng)
        out.append(_unit(name, "ov:" + name, dims, L, r, b))

    def three_at(k):  # run-0 pairs 0..k-1, then three runs of M at pairs k, k + 1, k + 2
        return np.concatenate([np.zeros(k, np.int64), [M, M, M]])

    add("first", [M])
    if nc > 10:
        add("one-round", three_at(10))
    else:
        add("one-round", three_at(min(3, nc)))  # the issue's 4x4x8 example, on the boxes this small
    if nc > 65:
        add("two-rounds", three_at(63))
    if nc > 1025:
        add("two-waves", three_at(1023))
    if nc > 4097:
        add("two-tiles", three_at(4095))
    if nc >= 3 * TILE:  # each tile's sum below 2^32, the first two together past it
        runs = np.zeros(2 * TILE, np.int64)
        runs[1500] = M
        runs[TILE + 700] = 2 ** 30
        runs[TILE + 3000] = 2 ** 30
        add("lookback", runs)
    add("all-sat", np.full(4100, M, np.int64))
    return out


# ------------------------------------------------------------- value bits --
def block_group(dims, bx, by, bz):
    """Flat positions of the eight coefficients of 2x2x2 block (bx, by, bz) of an
    even box: subband (sx, sy, sz) at (bx + sx W/2, by + sy H/2, bz + sz D/2)."""
    W, H, D = dims
    return [((bx + sx * (W // 2)) * H + by + sy * (H // 2)) * D + bz + sz * (D // 2)
            for sx in (0, 1) for sy in (0, 1) for sz in (0, 1)]


def value_units(dims, L, rng):
    W, H, D = dims
    nc = W * H * D
    out = []
    if nc == 0:
        return out
    n = nc  # every cell holds a pair
    zeros = np.zeros(n, np.uint32)
    out.append(_unit("random", "val:random", dims, L, zeros, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)))
    out.append(_unit("specials", "val:specials", dims, L, zeros, np.resize(PR.SPECIALS, n)))
    # whole blocks of -0.0 among finite values (even boxes), or every pair -0.0
    bits = _finite_bits(rng, n)
    if W % 2 == 0 and H % 2 == 0 and D % 2 == 0:
        for _ in range(max(1, nc // 64)):
            g = block_group(dims, int(rng.integers(0, W // 2)), int(rng.integers(0, H // 2)), int(rng.integers(0, D // 2)))
            bits[g] = 0x80000000
    else:
        bits[:] = 0x80000000
    out.append(_unit("-0-blocks", "val:-0-blocks", dims, L, zeros, bits))
    # explicit +0.0 pairs between pairs that skip cells
    m = max(1, nc // 3)
    bits = _finite_bits(rng, m)
    bits[rng.random(m) < 0.5] = 0
    bits[0] = 0
    out.append(_unit("+0", "val:+0", dims, L, rng.integers(0, 3, m), bits))
    bits = _finite_bits(rng, m)
    pick = rng.random(m) < 0.3
    bits[pick] = np.resize(NANS, int(pick.sum()))
    bits[:min(m, NANS.size)] = NANS[:min(m, NANS.size)]
    out.append(_unit("nan", "val:nan", dims, L, rng.integers(0, 3, m), bits))
    return out


# ------------------------------------------------------ region and coarse --
# (r, region) on the 32^3 box, None: the whole box (wc_inverse_coarse's region).
# tests/test_gpu_decode_payloads.py decodes every 32^3 unit over these.
def regions_of(dims, L):
    W, H, D = dims
    m = max(8, 1 << L)
    return [None, (W - m, 0, 0, m, H, D), (0, H - m, 0, W, m, D), (0, 0, D - m, W, H, m), (W - m, H - m, D - m, m, m, m)]


def end_of(dims, L, r, region):
    W, H, D = dims
    return int(G.index_map(dims, L, r, (0, 0, 0, W, H, D) if region is None else region)[2])


def end_units(dims, L, r, region, rng, tag):
    """Pairs at end - 1 and at end of one region's index map (the first position
    the region decoder no longer needs), and pair counts that put the pair at
    `end` on a tile boundary or one pair either side of it."""
    nc = dims[0] * dims[1] * dims[2]
    end = end_of(dims, L, r, region)
    out = []
    if end >= 1:
        pos = [end - 1] + ([end] if end < nc else [])
        out.append(_unit(f"end-last[{tag}]", "end:last", dims, L, _from_positions(pos), rng=rng))
    for d, name in ((-1, "tile-1"), (0, "tile"), (1, "tile+1")):
        cnt = TILE + d  # pairs below end: the pair at `end` has index cnt
        if cnt > end:
            continue
        hi = min(end + 100, nc)
        out.append(_unit(f"end-{name}[{tag}]", "end:" + name, dims, L, _from_positions(np.arange(end - cnt, hi)), rng=rng))
    return out


# (L, r, region index, region) of the end classes: the whole box at every r (the coarse
# decoder), the regions at r = 0 and 1; every region at L = 2, the first and the last at L = 1, 3
END_CASES = [(L, r, gi, g) for L in (1, 2, 3) for r in range(L + 1) for gi, g in enumerate(regions_of(CUBE, L))
             if (g is None or r < 2) and (L == 2 or gi in (0, 4))]


# ------------------------------------------------------------ the crafted set --
@functools.lru_cache(maxsize=None)
def crafted():
    """Every class on every box that reaches it, grouped by box."""
    rng = np.random.default_rng(16000)
    out = []
    for dims, L in BIG + SMALL:
        out += count_units(dims, L, rng)
        out += position_units(dims, L, rng)
        if dims[0] * dims[1] * dims[2]:
            out += overshoot_units(dims, L, rng)
    for dims, L in [(RIX, 1), (DENSE[1], 1), (CUBE, 2), (TINY[1], 1), (TINY[0], 1)]:
        out += value_units(dims, L, rng)
    for L, r, gi, g in END_CASES:
        out += end_units(CUBE, L, r, g, rng, f"r{r}g{gi}")
    names = [u.name for u in out]
    assert len(set(names)) == len(names)
    return tuple(out)


# ------------------------------------------------------------- classification --
def classify(u):
    """The classes a unit belongs to, from its runs (value classes: its bits) and box alone."""
    W, H, D = u.dims
    nc = W * H * D
    runs = u.runs.astype(np.int64)
    n = runs.size
    tags = set()
    if u.L >= 2:
        tags.add(f"levels:{u.L}")
    if not runs.any():
        if n in FIXED_COUNTS:
            tags.add(f"n={n}")
        if n - nc in REL_COUNTS:
            tags.add(f"n=nc{n - nc:+d}")
    if n == 0 or nc == 0:
        return tags
    pos = positions(runs)
    if n == 1 and pos[0] == nc - 1:
        tags.add("pos:last")
    if n == 1 and pos[0] == nc:
        tags.add("pos:dropped")
    if n == 4098 and pos[0] == nc - 1 and not runs[1:].any():
        tags.add("pos:last+4097")
    rows = np.arange(W * H, dtype=np.int64) * D
    if n == W * H and D > 1 and np.array_equal(pos, rows):
        tags.add("pos:row-starts")
    if n == W * H and D > 1 and np.array_equal(pos, rows + D - 1):
        tags.add("pos:row-ends")
    if np.array_equal(pos, np.arange(0, nc, 7 * D + 3)) and n > 1:
        tags.add("pos:sparse-rows")
    if n > TILE and not runs[:TILE].any() and runs[TILE] > 0 and pos[TILE] < nc and pos[TILE] // D == W * H - 1:
        tags.add("pos:tile-then-jump")
    if n >= 3 * TILE and n % TILE == 0 and pos[n - 2 * TILE] >= nc > pos[n - 2 * TILE - 1]:
        tags.add("pos:two-tiles-past")
    # overshoot: the exact sum before the trailing run-0 pairs is below ncoeff mod 2^32, and past it exactly
    trail = n - 1 - int(np.max(np.nonzero(runs)[0])) if runs.any() else 0
    if trail >= TRAIL:
        S = int(pos[n - trail - 1]) + 1
        if S > nc and S % 2 ** 32 < nc:
            big = np.nonzero(runs == M)[0]
            k = int(big[0]) if big.size else -1
            three = big.size >= 3 and big[1] == k + 1 and big[2] == k + 2
            if k == 0:
                tags.add("ov:first")
            if three and k // 64 == (k + 2) // 64:
                tags.add("ov:one-round")
            if three and k % 64 == 63 and k // 1024 == (k + 2) // 1024:
                tags.add("ov:two-rounds")
            if three and k % 1024 == 1023 and k // TILE == (k + 2) // TILE:
                tags.add("ov:two-waves")
            if three and k % TILE == TILE - 1:
                tags.add("ov:two-tiles")
            if big.size >= 4100 and np.array_equal(big[:4100], np.arange(4100)):
                tags.add("ov:all-sat")
            t = [int((runs[a:a + TILE] + 1).sum()) for a in range(0, n, TILE)]
            if len(t) >= 3 and max(t) < 2 ** 32 and t[0] < 2 ** 32 <= t[0] + t[1]:
                tags.add("ov:lookback")
    bits = u.bits
    if np.unique(bits >> np.uint32(24)).size > 200:
        tags.add("val:random")
    if np.isin(PR.SPECIALS, bits).all():
        tags.add("val:specials")
    if np.isin(NANS, bits).all():
        tags.add("val:nan")
    if (bits == 0).any():
        tags.add("val:+0")
    if W % 2 == 0 and H % 2 == 0 and D % 2 == 0 and n == nc and not runs.any():
        neg = bits.reshape(2, W // 2, 2, H // 2, 2, D // 2) == 0x80000000
        if neg.all(axis=(0, 2, 4)).any():  # all eight subband coefficients of some block
            tags.add("val:-0-blocks")
    elif (bits == 0x80000000).all():
        tags.add("val:-0-blocks")
    return tags


def classify_end(u, end):
    """The end classes of a unit for a region whose index map ends at `end`."""
    pos = positions(u.runs)
    n, tags = pos.size, set()
    if n == 0 or end < 1:
        return tags
    k = int(np.searchsorted(pos, end))  # the first pair at or past end
    if n <= 2 and pos[0] == end - 1 and (n == 1 or pos[1] == end):
        tags.add("end:last")
    at_end = k < n and pos[k] == end or end == u.ncoeff
    if k >= 1 and pos[k - 1] == end - 1 and at_end and k - TILE in (-1, 0, 1):
        tags.add(("end:tile-1", "end:tile", "end:tile+1")[k - TILE + 1])
    return tags


def is_overshoot(u):
    return any(t.startswith("ov:") for t in classify(u))


def is_surplus(u):
    """More pairs than cells: the surplus is dropped, whole tiles of it included."""
    return len(u.runs) > u.ncoeff


# ------------------------------------------------------------- fuzz batches --
def heavy_runs(rng, n, D):
    """Mostly 0..3, some up to D, a few up to 2^31 - 1."""
    c = rng.random(n)
    runs = rng.integers(0, 4, n)
    mid = (c >= 0.90) & (c < 0.995)
    runs[mid] = rng.integers(0, D + 1, int(mid.sum()))
    far = c >= 0.995
    runs[far] = rng.integers(0, 2 ** 31, int(far.sum()))
    return runs


FUZZ_SEEDS = (0, 1, 2)
FUZZ_DIMS = [RIX, DENSE[0], DENSE[1], CUBE, LONG] + TINY + [(8, 8, 8), (16, 8, 24), (6, 10, 14), (4, 4, 16), (16, 16, 16)]


def fuzz_batch(seed):
    """20-60 units: crafted classes drawn at random (one of each family at
    least), and random units on FUZZ_DIMS: L from the levels the box admits, a
    pair count from the classes or uniform up to ncoeff + 2 tiles, heavy-tailed
    runs (one unit in four: all 0), value bits uniform with a quarter specials."""
    rng = np.random.default_rng(16100 + seed)
    pool = crafted()  # shared: the units are never written to
    fam = {}
    for u in pool:
        fam.setdefault(u.cls.split(":")[0].split("=")[0], []).append(u)
    units = []
    for f in sorted(fam):
        for i in rng.choice(len(fam[f]), 3 if f in ("n", "pos", "ov") else 1, replace=False):
            units.append(fam[f][int(i)])
    total = int(rng.integers(20, 61))
    while len(units) < total:
        W, H, D = FUZZ_DIMS[int(rng.integers(0, len(FUZZ_DIMS)))]
        nc = W * H * D
        allowed = PR.levels_allowed(W, H, D) if nc else [1]
        L = allowed[int(rng.integers(0, len(allowed)))]
        counts = [c for c in FIXED_COUNTS if c <= nc + 2 * TILE] + [nc + d for d in REL_COUNTS if nc + d >= 0]
        n = int(rng.choice(counts)) if rng.random() < 0.5 else int(rng.integers(0, nc + 2 * TILE + 1))
        runs = np.zeros(n, np.int64) if rng.random() < 0.25 else heavy_runs(rng, n, D)
        units.append(_unit(f"s{seed}u{len(units)}n{n}", "fuzz", (W, H, D), L, runs, PR.value_bits(rng, n)))
    order = rng.permutation(len(units))
    return [units[int(i)] for i in order]


# -------------------------------------------------------------- the layout --
def payload_layout(pays, rng):
    """One buffer holding the payloads in another order, with gaps, at offsets
    that are 4 (mod 8) and 0 (mod 8) -> (uint8 buffer, uint64 offsets)."""
    order = rng.permutation(len(pays)) if len(pays) else []
    off = np.zeros(max(len(pays), 1), np.uint64)
    pos = 8 * int(rng.integers(1, 5))
    for j, i in enumerate(order):
        pos = (pos + 7) // 8 * 8 + (4 if (j + int(i)) % 2 == 0 else 0) + 8 * int(rng.integers(0, 4))
        off[i] = pos
        pos += len(pays[i])
    buf = np.full(pos + 16, 0xA5, np.uint8)  # the gaps hold no header
    for i, p in enumerate(pays):
        buf[int(off[i]):int(off[i]) + len(p)] = np.frombuffer(p, np.uint8)
    return buf, off


def cell_layout(cells, rng):
    """Output element offsets with gaps, every third at an odd offset
    (tests/test_gpu_fuzz.py _batch) -> (offsets, extent with a margin)."""
    offs, cur = [], 0
    for i, c in enumerate(cells):
        cur += int(rng.integers(0, 9))
        if i % 3 == 0 and cur % 2 == 0:
            cur += 1
        offs.append(cur)
        cur += c
    return offs, cur + 8
