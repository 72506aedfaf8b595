"""numpy restatement of the packed payload format and of its value rule q
(include/wavelet_amd.h, "Opt-in packed payloads").  TEST INFRASTRUCTURE ONLY:
the yardstick of tests/test_pack_cpu.py, tests/test_gpu_pack.py and
tests/test_gpu_pack_fuzz.py; the product never imports it.  pack() and unpack()
loop over chunks in plain numpy: about 1.6 s and 1.5 s for the 2^21 pairs of
limit_unit(), which the tests restate once, at one V.

A standard payload is 20 bytes of header (int32 W, H, D, ncoeff, nrle) and nrle
pairs {int32 run, fp32 value}.  A packed unit: the header with ncoeff replaced by
tag = -(16 V + L), a width table of ceil(n / 64) bytes padded to a multiple of 8,
then per chunk of 64 pairs w_c bit planes of the runs and V byte planes of the
values' top bytes.
"""
import numpy as np

import levels_ref as LR
from tol_rule import field

MAX_LEVELS = 4
TILE = 2048  # pairs per transcoder workgroup (csrc/wc_internal.h kPackTile)


def q(bits, V):
    """The value rule on uint32 bit patterns (array or scalar) -> uint32 array."""
    b = np.atleast_1d(np.asarray(bits, np.uint64)) & np.uint64(0xFFFFFFFF)
    if V == 4:
        return b.astype(np.uint32)
    s = np.uint64(8 * (4 - V))
    low = (np.uint64(1) << s) - np.uint64(1)
    keep = np.uint64(0xFFFFFFFF) ^ low
    m = b & np.uint64(0x7FFFFFFF)
    sign = b & np.uint64(0x80000000)
    r = (m + (np.uint64(1) << (s - np.uint64(1))) - np.uint64(1) + ((m >> s) & np.uint64(1))) & keep
    r = np.where(r >= np.uint64(0x7F800000), m & keep, r)
    out = sign | r
    out = np.where(m == np.uint64(0x7F800000), b, out)
    out = np.where(m > np.uint64(0x7F800000), (b | np.uint64(0x00400000)) & keep, out)
    return out.astype(np.uint32)


def tag(L, V):
    return -(16 * V + L)


def pad8(v):
    return (v + 7) // 8 * 8


def parse(pay):
    """A standard payload -> (W, H, D, L, runs uint32[n], value bits uint32[n])."""
    h = np.frombuffer(pay[:20], np.int32)
    W, H, D, nc, n = (int(v) for v in h)
    L = 1 if nc >= 0 else -nc
    assert (nc == W * H * D) or (2 <= -nc <= MAX_LEVELS), nc
    assert len(pay) == 20 + 8 * n
    pairs = np.frombuffer(pay[20:], np.uint32).reshape(n, 2)
    return W, H, D, L, pairs[:, 0].copy(), pairs[:, 1].copy()


def standard(W, H, D, L, runs, bits):
    pairs = np.empty((len(runs), 2), np.uint32)
    pairs[:, 0] = runs
    pairs[:, 1] = bits
    head = np.array([W, H, D, W * H * D if L == 1 else -L, len(runs)], np.int32)
    return head.tobytes() + pairs.tobytes()


def quantise(pay, V):
    """The standard payload wc_unpack(wc_pack(pay, V)) must give."""
    W, H, D, L, runs, bits = parse(pay)
    return standard(W, H, D, L, runs, q(bits, V))


def pack(pay, V):
    W, H, D, L, runs, bits = parse(pay)
    n = len(runs)
    assert n <= W * H * D and not (runs >> 31).any()
    nch = (n + 63) // 64
    qb = q(bits, V) if n else np.zeros(0, np.uint32)
    table = np.zeros(pad8(nch), np.uint8)
    body = []
    for c in range(nch):
        r = runs[64 * c:64 * c + 64]
        v = qb[64 * c:64 * c + 64]
        m = len(r)
        w = int(np.bitwise_or.reduce(r)).bit_length()
        table[c] = w
        for b in range(w):
            body.append(np.packbits(((r >> np.uint32(b)) & np.uint32(1)).astype(np.uint8), bitorder="little").tobytes())
            assert len(body[-1]) == (m + 7) // 8
        for p in range(V):
            body.append(((v >> np.uint32(8 * (3 - p))) & np.uint32(0xFF)).astype(np.uint8).tobytes())
    head = np.array([W, H, D, tag(L, V), n], np.int32)
    return head.tobytes() + table.tobytes() + b"".join(body)


def packed_size(packed):
    h = np.frombuffer(packed[:20], np.int32)
    n = int(h[4])
    V = (-int(h[3])) >> 4
    nch = (n + 63) // 64
    total = 20 + pad8(nch)
    for c in range(nch):
        m = 64 if c + 1 < nch else n - 64 * (nch - 1)
        total += packed[20 + c] * ((m + 7) // 8) + V * m
    return total


def unpack(packed):
    h = np.frombuffer(packed[:20], np.int32)
    W, H, D, t, n = (int(v) for v in h)
    V, L = (-t) >> 4, (-t) & 15
    nch = (n + 63) // 64
    pos = 20 + pad8(nch)
    runs, bits = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for c in range(nch):
        m = 64 if c + 1 < nch else n - 64 * (nch - 1)
        pl = (m + 7) // 8
        for b in range(packed[20 + c]):
            plane = np.unpackbits(np.frombuffer(packed[pos:pos + pl], np.uint8), bitorder="little")[:m]
            runs[64 * c:64 * c + m] |= plane.astype(np.uint32) << np.uint32(b)
            pos += pl
        for p in range(V):
            bits[64 * c:64 * c + m] |= np.frombuffer(packed[pos:pos + m], np.uint8).astype(np.uint32) << np.uint32(8 * (3 - p))
            pos += m
    assert pos == len(packed)
    return standard(W, H, D, L, runs, bits)


def worst(N, V):
    """S(N): the worst-case packed unit of N cells."""
    return 20 + pad8((N + 63) // 64) + 31 * ((N + 7) // 8) + V * N


def slot_offsets(dims, V):
    """Unit u's slot in the packed buffer, and the capacity (wc_packed_bound)."""
    off = [4]
    for W, H, D in dims:
        off.append(off[-1] + pad8(worst(W * H * D, V) + 4))
    return off[:-1], off[-1]


def payload_slots(dims):
    """Unit u's slot in the standard payload buffer, and wc_payload_bound."""
    off = [4]
    for W, H, D in dims:
        off.append(off[-1] + 24 + 8 * W * H * D)
    return off[:-1], off[-1]


# ---------------------------------------------------------------- the batch --
# (what, dims, L, field kind, pairs wanted or None)
SPECIALS = np.array([
    0x3F808000, 0x3F818000, 0x3F800080, 0x3F800180,  # ties at V = 2 and at V = 3, both directions
    0x3FFFFFFF, 0x407FFFFF, 0x7F7FFFFF, 0xFF7FFFFF,  # all-ones mantissas (carry into the exponent), +-FLT_MAX
    0x7F800000, 0xFF800000, 0x7F800001, 0xFFC00000, 0x7FBFFFFF, 0x7F80FFFF,  # +-inf, NaNs
    0x00000001, 0x80000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x807F8000,  # subnormals
    0x00000000, 0x80000000, 0x00800000, 0x3F800000, 0xBF800000, 0x7F7F8000, 0x7F7FFF80,
], np.uint32)


def with_pairs(box, L, K):
    """A payload of `box` at L levels with exactly K pairs (an explicit threshold)."""
    flat = LR.decompose(box, L)
    a = np.sort(np.abs(flat))[::-1]
    t = float(a[K]) if K < a.size else -1.0
    if K == 0:
        t = float(a[0])
    pay, kept = LR.payload(box, L, thresh=t) if t >= 0 else (None, None)
    assert pay is not None and kept == K, (box.shape, L, K, kept)
    return pay


def crafted():
    """Payloads of an 8^3 unit made by hand: wide runs, a chunk of mixed widths, special values."""
    rng = np.random.default_rng(9100)
    out = []
    # runs up to 0x7FFFFFFF (w = 31), 130 pairs
    runs = rng.integers(0, 1 << 31, 130, dtype=np.uint64).astype(np.uint32)
    runs[7] = 0x7FFFFFFF
    out.append(("w31", standard(8, 8, 8, 1, runs, rng.integers(0, 1 << 32, 130, dtype=np.uint64).astype(np.uint32))))
    # one chunk of mixed widths (lane j has j % 32 bits), then a chunk of zeros, then a short one
    runs = np.concatenate([(np.uint64(1) << (np.arange(64, dtype=np.uint64) % 31)).astype(np.uint32),
                           np.zeros(64, np.uint32), np.array([5, 0, 300], np.uint32)])
    out.append(("mixed", standard(8, 8, 8, 2, runs, np.resize(SPECIALS, runs.size))))
    # the special values, twice over, in 512 pairs: the unit's cell count
    out.append(("specials", standard(8, 8, 8, 3, np.arange(512, dtype=np.uint32) % 3, np.resize(SPECIALS, 512))))
    return out


NATURAL = [
    # what, (W, H, D), L, kind, pairs
    ("n0", (8, 8, 8), 1, 0, 0), ("n1", (8, 8, 8), 2, 2, 1), ("n63", (8, 8, 8), 3, 0, 63),
    ("n64", (16, 8, 8), 1, 2, 64), ("n65", (16, 8, 8), 2, 0, 65), ("n128", (16, 16, 8), 3, 1, 128),
    ("tile-1", (32, 16, 8), 1, 1, TILE - 1), ("tile", (32, 16, 8), 2, 1, TILE), ("tile+1", (32, 16, 8), 3, 1, TILE + 1),
    ("odd", (16, 16, 16), 2, 0, 777), ("front", (8, 16, 8), 1, 2, 300),
]


def batch(src="f32"):
    """-> list of (what, payload bytes, finite: the values are all finite and the
    unit is one of the field units).  src: "f32" fields as they are, "f64" fields
    made in double precision and narrowed."""
    from oracle import oracle as O
    units = []
    for i, (what, (W, H, D), L, kind, K) in enumerate(NATURAL):
        box = field(kind, W, H, D, 9000 + i)
        if src == "f64":
            box = O.narrow(box.astype(np.float64) * (1.0 + 2.0 ** -30) + 2.0 ** -31)
        units.append((what, with_pairs(box, L, K), True))
    units.append(("empty", LR.payload(np.zeros((0, 4, 4), np.float32), 1, keep=0.5)[0], True))
    noise = field(1, 16, 8, 8, 9050)
    units.append(("all", LR.payload(noise, 1, thresh=0.0)[0], True))  # fully kept: every run 0, every w_c = 0
    units.append(("const", LR.payload(field(3, 8, 8, 8, 9051), 2, keep=0.999)[0], True))
    units += [(w, p, False) for w, p in crafted()]
    big = field(0, 64, 64, 64, 9060)
    if src == "f64":
        big = O.narrow(big.astype(np.float64) * (1.0 + 2.0 ** -30))
    units.append(("64^3", LR.payload(big, 1, keep=0.999)[0], True))
    return units


# ------------------------------------------------------------- the fuzz units --
# Units for the transcoders alone, made with standard() as crafted() makes its
# own: the runs need not fit the box, so no decoder reads them (finite = False).
FUZZ_DIMS = [(1, 1, 1), (2, 2, 2), (3, 5, 7), (5, 1, 9), (6, 10, 14), (33, 17, 9), (0, 4, 4), (8, 8, 8), (16, 16, 16),
             (24, 8, 40), (64, 32, 16)]
FULL_DIMS = [(2, 2, 2), (3, 5, 7), (8, 8, 8), (6, 10, 14)]  # cells 8, 105, 512, 840: 105 % 8 and 840 % 64 are not 0
FUZZ_SEEDS = (0, 1, 2)
FUZZ_DRAWN = 40
MANY_DIMS = [(2, 2, 2), (1, 1, 1), (0, 4, 4), (3, 5, 7), (4, 4, 4), (8, 8, 8)]
LIMIT_DIMS = (128, 128, 128)  # WC_PACK_MAX_CELLS = 2^21 cells


def levels_allowed(W, H, D):
    """The L a header of this box may carry: 1, and every L <= 4 whose 2^L divides each dimension."""
    return [L for L in range(1, MAX_LEVELS + 1) if L == 1 or (W | H | D) & ((1 << L) - 1) == 0]


def chunk_widths(pay):
    """-> (the width of every chunk, the pairs in the last chunk) of a standard payload."""
    runs = parse(pay)[4]
    nch = (len(runs) + 63) // 64
    w = [int(np.bitwise_or.reduce(runs[64 * c:64 * c + 64])).bit_length() for c in range(nch)]
    return w, (len(runs) - 64 * (nch - 1) if nch else 0)


def runs_of_widths(rng, n, widths):
    """n runs whose chunk c has the width widths[c] exactly: every run below 2^w, one of them with bit w - 1 set."""
    runs = np.zeros(n, np.uint32)
    for c, w in enumerate(widths):
        m = min(64, n - 64 * c)
        if w:
            r = rng.integers(0, 1 << int(w), m, dtype=np.uint64)
            r[rng.integers(0, m)] |= np.uint64(1) << np.uint64(int(w) - 1)
            runs[64 * c:64 * c + m] = r.astype(np.uint32)
    return runs


def value_bits(rng, n, share=0.25):
    """n uniform uint32 bit patterns, `share` of them from SPECIALS."""
    bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    pick = rng.random(n) < share
    bits[pick] = SPECIALS[rng.integers(0, SPECIALS.size, int(pick.sum()))]
    return bits


class _Deck:
    """The widths 0..31 dealt without replacement and reshuffled when none is left: 63 draws hold every width."""

    def __init__(self, rng):
        self.rng, self.left = rng, []

    def draw(self):
        if not self.left:
            self.left = self.rng.permutation(32).tolist()
        return self.left.pop()


def pair_count(rng, cells, cls):
    """A pair count of class cls (0..15; 10 and above: uniform), clipped to the cell count."""
    k64, k2048 = int(rng.integers(1, max(cells // 64, 1) + 1)), int(rng.integers(1, max(cells // TILE, 1) + 1))
    n = [0, 1, cells, cells - 1, 64 * k64 - 1, 64 * k64, 64 * k64 + 1, TILE * k2048 - 1, TILE * k2048, TILE * k2048 + 1,
         int(rng.integers(0, cells + 1))][min(cls, 10)]
    return min(max(n, 0), cells)


def fuzz_batch(seed):
    """-> FUZZ_DRAWN + len(FULL_DIMS) units (what, payload, False).  The drawn
    ones: dimensions from FUZZ_DIMS (each at least three times), L from
    levels_allowed, a pair count of one of eleven classes (pair_count; the unit
    index walks them, the uniform one six times in sixteen), per chunk a width from a deck of 0..31 (one deck for
    the full chunks, one for the short last chunks) or, one time in eight, an
    all-zero chunk; value bits uniform with a quarter from SPECIALS.  Then the full
    slots: n = cells and every width 31 on FULL_DIMS."""
    rng = np.random.default_rng(9300 + seed)
    full, last = _Deck(rng), _Deck(rng)
    order = [FUZZ_DIMS[i % len(FUZZ_DIMS)] for i in rng.permutation(FUZZ_DRAWN)]
    units = []
    for i, (W, H, D) in enumerate(order):
        cells = W * H * D
        allowed = levels_allowed(W, H, D)
        L = allowed[int(rng.integers(0, len(allowed)))]
        n = pair_count(rng, cells, (i + 5 * seed) % 16)
        nch = (n + 63) // 64
        widths = [0 if rng.random() < 0.125 else full.draw() for _ in range(nch)]
        if n % 64:
            widths[-1] = last.draw()
        units.append((f"s{seed}u{i}:{W}x{H}x{D}/L{L}/n{n}",
                      standard(W, H, D, L, runs_of_widths(rng, n, widths), value_bits(rng, n)), False))
    for W, H, D in FULL_DIMS:
        n = W * H * D
        units.append((f"s{seed}full:{W}x{H}x{D}", standard(W, H, D, 1, runs_of_widths(rng, n, [31] * ((n + 63) // 64)),
                                                          value_bits(rng, n)), False))
    return units


def many_units(count):
    """-> `count` tiny units (what, payload, False), each list a prefix of the
    longer ones: dimensions cycling over MANY_DIMS, n uniform in 0..cells (so the
    lengths vary; the units without cells and the draws of n = 0 are bare 20-byte
    headers), widths uniform in 0..12."""
    rng = np.random.default_rng(9400)
    units = []
    for i in range(count):
        W, H, D = MANY_DIMS[i % len(MANY_DIMS)]
        n = int(rng.integers(0, W * H * D + 1))
        widths = rng.integers(0, 13, (n + 63) // 64)
        units.append((f"m{i}:{W}x{H}x{D}/n{n}", standard(W, H, D, 1, runs_of_widths(rng, n, widths), value_bits(rng, n)),
                      False))
    return units


def limit_unit(n):
    """-> one unit (what, payload, False) of 128^3 cells (WC_PACK_MAX_CELLS) at L = 1
    with n pairs: runs below 2^12, one chunk in sixteen all zero, value bits uniform."""
    rng = np.random.default_rng(9500 + n % 9973)
    W, H, D = LIMIT_DIMS
    runs = rng.integers(0, 1 << 12, n, dtype=np.uint64).astype(np.uint32)
    zero = np.repeat(rng.random((n + 63) // 64) < 1.0 / 16, 64)[:n]
    runs[zero] = 0
    return (f"limit/n{n}", standard(W, H, D, 1, runs, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)), False)
