"""The crafted decoder payloads (tests/decode_payloads.py) on the CPU: the set
the GPU test decodes holds every class, the oracle decodes each payload as the
project's rule in Python ints does, and two wrong models of the scan (a
wrapping 32-bit sum, a saturating one without the clamp to ncoeff) disagree
with the oracle on every overshoot payload while the decoders' own arithmetic
(saturating, clamped) agrees on every payload.  No GPU."""
import numpy as np
import pytest

import coarse_ref as C
import decode_payloads as DP
import levels_ref as LR
import region_ref as G


@pytest.fixture(scope="module")
def units():
    out = list(DP.crafted())
    for s in DP.FUZZ_SEEDS:
        out += DP.fuzz_batch(s)
    return out


def test_every_class_is_present(units):
    """Class membership from the runs (the value classes: from the bits) alone, over
    the crafted set and the fuzz seeds the GPU test runs."""
    found = {}
    for u in units:
        for t in DP.classify(u):
            found.setdefault(t, []).append(u.name)
    for L, r, gi, g in DP.END_CASES:
        end = DP.end_of(DP.CUBE, L, r, g)
        for u in units:
            if u.dims == DP.CUBE and u.L == L:
                for t in DP.classify_end(u, end):
                    found.setdefault(t, []).append(u.name)
    missing = [c for c in DP.ALL_CLASSES if c not in found]
    assert not missing, missing
    print({c: len(found[c]) for c in DP.ALL_CLASSES})
    # every unit on a box with pair tiles is in the class it was built for
    big = {d for d, _ in DP.BIG}
    for u in DP.crafted():
        if u.dims in big and not u.cls.startswith("end:") and u.cls != "val:random":
            assert u.cls in DP.classify(u), u.name
    # every end class at every region and reduction the GPU test decodes
    for L, r, gi, g in DP.END_CASES:
        end = DP.end_of(DP.CUBE, L, r, g)
        mine = [u for u in DP.crafted() if u.cls.startswith("end:") and u.L == L and f"[r{r}g{gi}]" in u.name]
        got = {u.cls for u in mine if u.cls in DP.classify_end(u, end)}
        want = {"end:last"} | ({"end:tile-1", "end:tile", "end:tile+1"} if end > DP.TILE else set())
        assert got >= want, (L, r, gi, end, got)
    # the boxes: every count class on every box with that many cells, every fuzz batch within its size
    for dims, L in DP.BIG:
        nc = dims[0] * dims[1] * dims[2]
        mine = {len(u.runs) for u in DP.crafted() if u.dims == dims and u.L == L and not u.runs.any()}
        assert mine >= {n for n in DP.FIXED_COUNTS if n <= nc} | {nc + d for d in DP.REL_COUNTS}, dims
    for s in DP.FUZZ_SEEDS:
        b = DP.fuzz_batch(s)
        assert 20 <= len(b) <= 60
        runs = np.concatenate([u.runs for u in b if u.cls == "fuzz"])
        assert (runs <= 3).mean() > 0.8 and (runs > 2288).any() and (runs >= 2 ** 30).any()  # the heavy tail
    # valid payloads only: the unit's header, nrle >= 0, no negative run
    for u in units:
        h = np.frombuffer(u.payload[:20], "<i4")
        assert tuple(h[:3]) == u.dims and h[3] == (u.ncoeff if u.L == 1 else -u.L) and h[4] == len(u.runs) >= 0
        assert not (u.runs >> np.uint32(31)).any()


def test_layouts_are_what_the_header_allows():
    rng = np.random.default_rng(5)
    pays = [u.payload for u in DP.fuzz_batch(0)]
    buf, off = DP.payload_layout(pays, rng)
    o = off[:len(pays)].astype(np.int64)
    assert (o % 4 == 0).all() and (o % 8 == 4).any() and (o % 8 == 0).any()
    assert list(o) != sorted(o) and int(o.min()) >= 8  # another order, nothing at the buffer's start
    spans = sorted((int(a), int(a) + len(p)) for a, p in zip(o, pays))
    assert all(b0 <= a1 for (_, b0), (a1, _) in zip(spans, spans[1:])) and spans[-1][1] <= buf.size
    assert any(a1 > b0 for (_, b0), (a1, _) in zip(spans, spans[1:]))  # gaps
    for a, p in zip(o, pays):
        assert buf[a:a + len(p)].tobytes() == p
    offs, ext = DP.cell_layout([8, 0, 27, 64], rng)
    assert offs[0] % 2 == 1 and offs[3] % 2 == 1 and ext >= offs[3] + 64 + 8


def test_oracle_follows_the_rule(oracle, units):
    """wco_rle_decode (a 64-bit index) = the rule in Python ints, bit for bit, on
    every payload; and through the references the GPU test compares with."""
    for u in units:
        if u.ncoeff == 0:
            continue
        (W, H, D), nc, runs, vals = oracle.parse_payload(u.payload)
        assert (W, H, D) == u.dims and np.array_equal(runs.view(np.uint32), u.runs)
        assert np.array_equal(vals.view(np.uint32), u.bits)  # NaN payloads and signs survive the parse
        got = oracle.rle_decode(runs, vals, u.ncoeff).view(np.uint32)
        assert np.array_equal(got, DP.rule_decode(u.runs, u.bits, u.ncoeff)), u.name
    # the issue's example: one coefficient, at position 3
    ex = DP.Unit("ex", "", (4, 4, 8), 1, np.array([3, DP.M, DP.M, DP.M, 0, 0, 0], np.uint32), np.arange(1, 8, dtype=np.uint32))
    flat = oracle.rle_decode(ex.runs.view(np.int32), ex.bits.view(np.float32), 128).view(np.uint32)
    assert np.nonzero(flat)[0].tolist() == [3] and flat[3] == 1
    # a -0.0 pair is not the zero fill, and survives synthesis where a whole block is -0.0
    neg = [u for u in units if u.cls == "val:-0-blocks"]
    assert len(neg) >= 4
    for u in neg:
        assert (DP.rule_decode(u.runs, u.bits, u.ncoeff) == 0x80000000).any(), u.name
        if u.L == 1:  # (at L >= 2 a block's average is a level-2 result, not a pair)
            assert (oracle.decompress_payload(u.payload).view(np.uint32) == 0x80000000).any(), u.name
    assert sum(u.L == 1 for u in neg) >= 3 and LR.decode(neg[0].payload)[1] == neg[0].L


def _sums(runs, sat):
    """Inclusive sums of run + 1 in 32 bits: wrapping, or saturating at 2^32 - 1."""
    s = np.cumsum(runs.astype(np.uint64) + np.uint64(1))
    if not sat:
        return (s & np.uint64(0xFFFFFFFF)).astype(np.int64)
    # a saturating sum of non-negative terms is the exact sum, clamped: once at the clamp it stays
    return np.minimum(s, np.uint64(0xFFFFFFFF)).astype(np.int64)


def _model(u, sat, clamp):
    """Pair positions as a 32-bit scan sees them (a dropped pair at ncoeff when it
    clamps), and the flat array a decoder writing `position < ncoeff` gives."""
    nc = u.ncoeff
    pos = (_sums(u.runs, sat) - 1) & 0xFFFFFFFF
    if clamp:
        pos = np.minimum(pos, nc)
    flat = np.zeros(nc, np.uint32)
    if sat:  # positions below ncoeff are exact and increase: no cell is written twice
        flat[pos[pos < nc]] = u.bits[pos < nc]
        return pos, flat
    for p, b in zip(pos.tolist(), u.bits.tolist()):  # in pair order: a later pair overwrites
        if p < nc:
            flat[p] = b
    return pos, flat


def test_wrong_scans_disagree_on_every_overshoot(oracle, units):
    """A wrapping uint32 sum writes overshoot pairs into the box; a saturating sum
    without min(., ncoeff) names rows past the row table (k_rowindex divides the
    position by D).  The saturating, clamped sum is the oracle on every payload."""
    seen = set()
    for u in units:
        if u.ncoeff == 0 or len(u.runs) == 0:
            continue
        W, H, D = u.dims
        want_flat = oracle.rle_decode(u.runs.view(np.int32), u.bits.view(np.float32), u.ncoeff).view(np.uint32)
        want_pos = np.minimum(DP.positions(u.runs), u.ncoeff)  # a dropped pair counts as position ncoeff
        pos, flat = _model(u, sat=True, clamp=True)
        assert np.array_equal(pos, want_pos) and np.array_equal(flat, want_flat), u.name
        assert int(pos.max()) // D <= W * H  # inside the row table, sentinel row included
        ov = {t for t in DP.classify(u) if t.startswith("ov:")}
        if not ov:
            continue
        seen |= ov
        wpos, wflat = _model(u, sat=False, clamp=False)
        assert not np.array_equal(wflat, want_flat), u.name
        assert (wflat == DP.MARK).any() and not (want_flat == DP.MARK).any(), u.name  # the trailing pairs land inside
        spos, sflat = _model(u, sat=True, clamp=False)
        assert not np.array_equal(spos, want_pos) and int(spos.max()) // D > W * H, u.name
    assert seen == set(DP.OVERSHOOT)
    # every overshoot class on every box with pair tiles
    for dims, L in DP.BIG:
        got = set()
        for u in DP.crafted():
            if u.dims == dims and u.L == L:
                got |= {t for t in DP.classify(u) if t.startswith("ov:")}
        assert got >= set(DP.OVERSHOOT) - ({"ov:lookback"} if dims == DP.LONG else set()), (dims, L, got)


def test_region_ends_match_the_index_map():
    """end_units puts its pairs where region_ref's map ends: the pair at end - 1 is
    kept by the map of its region, no position at or past end is."""
    for L, r, gi, g in DP.END_CASES:
        W, H, D = DP.CUBE
        p, _, end = G.index_map(DP.CUBE, L, r, (0, 0, 0, W, H, D) if g is None else g)
        assert p.size and int(p.max()) == end - 1, (L, r, gi)
        assert end == DP.end_of(DP.CUBE, L, r, g)
    # the whole box at r = 0 ends at ncoeff; a far-corner block too; the first x slab does not
    assert DP.end_of(DP.CUBE, 2, 0, None) == 32 ** 3 == DP.end_of(DP.CUBE, 2, 0, DP.regions_of(DP.CUBE, 2)[4])
    assert DP.end_of(DP.CUBE, 2, 1, None) < 32 ** 3
    assert C.payload_levels(DP.crafted()[0].payload) == 1
