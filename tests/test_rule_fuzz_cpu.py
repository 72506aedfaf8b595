"""CPU: the seeded cases of the rule-driven modes (rule_fuzz.py, maxerr_tiles.py,
pairs_fuzz.tol_batch) through the host rules, and the proof that the cases hold what
tests/test_gpu_maxerr_fuzz.py, tests/test_gpu_leveltol_fuzz.py and
tests/test_gpu_pairs_tol_fuzz.py rely on.  Seeds 0 and 1, the seeds the GPU tests run
by default.

The host rules (wc_maxerr_select, wc_tol_levels_threshold on
leveltol_rule.level_counts, wc_thin_tol_unit, wc_split_tol_unit) must equal the
restatements bit for bit.  The class counts are floors that keep a GPU test from
passing on an empty class.  Measured on seed 0 / seed 1 (floor):

  max-error bound, 37 / 42 units: b* = 0: 9 / 9 (4); 0 < b* < 4095: 16 / 20 (4);
    b* = 4095: 12 / 13 (4); units with cells at an odd cell offset: 28 / 28 (8).
    A batch holds one bound per unit, so a unit drawn as kind 6 (E = err(b) of a
    random bin) or 7 (the double below it) carries a twin decision, the search under
    the other bound of the two; restatement and host rule run both.  The twin ends at
    another b* on 9 of 9 / 8 of 8 such units (3).
  per-level tolerance: units that keep some but not all non-zero coefficients:
    11 / 10 (3); walks that stop at a level > 1: 1 / 2 (1: the class must occur).
  thin / split to a tolerance: 14 of 23 / 15 of 22 units accepted; of these, with P
    the pairs a zero tolerance keeps (the live pairs that are not +-0 or NaN): some
    but not all of P kept: 8 / 9 (5); none kept: 4 / 3, of which P is not empty on
    1 / 0 (1 on the former count); all of P > 0 kept: 2 / 3 (1); pairs past N: 2 / 5
    (1); a NaN pair below N: 8 / 9 (1)."""
import numpy as np
import pytest

import layers_rule as LR
import levels_ref as R
import leveltol_rule as LT
import maxerr_rule as MR
import maxerr_tiles as MT
import pairs_fuzz as PF
import rule_fuzz as RF
import thin_rule as TR
import thin_tol_rule as TT
from tol_rule import same_bits

SEEDS = (0, 1)


@pytest.mark.parametrize("seed", SEEDS)
def test_maxerr_batches_through_the_host_rule(wc, oracle, seed):
    B = RF.maxerr_case(wc.capi, oracle, seed)
    assert B.dtype == (np.float64 if seed % 2 == 0 else np.float32)
    bs = [w[4] for w in B.want]
    moved = 0
    for i in range(B.n):
        W, H, D = B.dims[i]
        who = (seed, i, B.dims[i], B.levels[i], B.kind[i], B.E[i])
        assert W * H * D == 0 or not (W | H | D) & 1, who
        for E, b in ((B.E[i], bs[i]),) + ((B.twin[i],) if B.twin[i] else ()):
            gt, ge, gb = wc.capi.maxerr_select(B.flat[i], B.x[i], B.dims[i], B.levels[i], E)
            assert gb == b, (who, E, gb, b)
            assert same_bits(gt, float(MR.thr(b)), np.float32), (who, E)
            if E == B.E[i]:
                assert same_bits(ge, B.want[i][3]), (who, ge, B.want[i][3])
                assert gb == 0 or ge <= E, who
        if B.twin[i]:
            assert B.kind[i] in (6, 7) and B.twin[i][0] != B.E[i]
            lo, hi = sorted((B.E[i], B.twin[i][0]))
            assert np.nextafter(hi, 0.0) == lo
            moved += B.twin[i][1] != bs[i]
    odd = sum(B.units[i].cell_offset % 2 and B.x[i].size > 0 for i in range(B.n))
    n0, nmid, ntop = sum(b == 0 for b in bs), sum(0 < b < 4095 for b in bs), sum(b == 4095 for b in bs)
    print(f"maxerr seed {seed}: n {B.n} b*=0 {n0} mid {nmid} top {ntop} odd {odd} twins moved {moved} "
          f"of {sum(t is not None for t in B.twin)} kinds {sorted(set(B.kind))}")
    assert min(n0, nmid, ntop) >= 4 and moved >= 3 and odd >= 8
    assert set(B.kind) == set(range(8))
    # the cells of both kinds of pointer: units whose cells start off a 2 * sizeof(T) boundary, and on one
    assert any(B.units[i].cell_offset % 2 == 0 and B.x[i].size for i in range(B.n))


def _tile_classes(dims, ty):
    axes = MT.tiles(dims, ty)
    return tuple(len(a) for a in axes), tuple(a[-1][1] for a in axes)


def test_tile_shapes_show_the_classes_of_the_table():
    for dims, L in MT.SHAPES:
        for ty, want in MT.TABLE[dims].items():
            assert L < 4 or ty == 16
            got = _tile_classes(dims, ty)
            assert got == want, (dims, ty, got)
            for n, edge, (count, last) in zip(dims, (MT.TX, ty, MT.TZ), zip(*got)):
                assert (count - 1) * edge + last == n and 0 < last <= edge and last % (1 << L) == 0 and edge % (1 << L) == 0
        assert (16 in MT.TABLE[dims]) and ((8 in MT.TABLE[dims]) == (L < 4))
    clips8 = {d: _tile_classes(d, 8)[1] for d, L in MT.SHAPES if L < 4}
    # every admissible clip under TY = 8: the multiples of 2^L below the tile's edge that some L <= 3 admits
    assert {c[0] for c in clips8.values()} >= {2, 4, 8, 12, 14, 16}
    assert {c[1] for c in clips8.values()} >= {2, 4, 6, 8}
    assert {c[2] for c in clips8.values()} >= {2, 4, 8, 24, 28, 30, 32}
    for dims, blocks in MT.ODD_BLOCKS.items():
        L = dict(MT.SHAPES)[dims]
        assert tuple((e >> 1) >> (L - 1) for e in clips8[dims]) == blocks
        assert sum(len(a) > 1 and b % 2 == 1 for a, b in zip(MT.tiles(dims, 8), blocks)) >= 1
    assert tuple(e >> 1 for e in clips8[(30, 14, 62)]) == (7, 3, 15)
    # a clipped tile off the origin on every axis, and a clipped y tile at L = 3 under TY = 16
    assert all(any(_tile_classes(d, 8)[0][a] > 1 and _tile_classes(d, 8)[1][a] < e for d, L in MT.SHAPES if L == 3)
               for a, e in ((0, MT.TX), (2, MT.TZ)))
    assert _tile_classes((24, 24, 40), 16) == ((2, 2, 2), (8, 8, 8)) and dict(MT.SHAPES)[(24, 24, 40)] == 3
    sizes = {ty: sum(u.box.size for u in MT.units(ty)) for ty in (8, 16)}
    print("tile lists:", {ty: (len(MT.units(ty)), sizes[ty]) for ty in sizes})
    assert max(sizes.values()) <= 3 << 19  # a call stays at half of a levels batch


class _Blind(MR.Unit):
    """The unit with the target tile's cells left out of the max."""

    def __init__(self, x, flat, L, seen):
        super().__init__(x, flat, L)
        self.seen = seen.ravel()

    def err(self, b):
        if b not in self.memo:
            self.memo[b] = MR.max_abs(self.x.ravel()[self.seen], self.recon(b).ravel()[self.seen])
        return self.memo[b]


@pytest.mark.parametrize("maxl", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tile_units_through_the_host_rule(wc, oracle, maxl, dtype):
    B = RF.tiles_case(wc.capi, oracle, maxl, dtype, odd=False)
    O = RF.tiles_case(wc.capi, oracle, maxl, dtype, odd=True)
    assert O.want == B.want and B.cells.tobytes() != O.cells.tobytes()
    assert all(B.units[i].cell_offset % 4 == 0 for i in range(B.n))
    ty = MT.ty_of(maxl)
    for i, u in enumerate(B.us):
        pay, kept, t, e, b = B.want[i]
        who = (maxl, dtype.__name__, u.name)
        flat = R.decompose(B.boxes[i], u.L)
        gt, ge, gb = wc.capi.maxerr_select(flat, B.x[i], u.dims, u.L, B.E[i])
        assert gb == b and same_bits(gt, float(t), np.float32) and same_bits(ge, e), (who, gb, b, ge, e)
        assert 0 < b < 4095 and 0.0 < e <= B.E[i], (who, b, e)
        if dtype == np.float64:
            assert B.x[i].astype(np.float32).astype(np.float64).tobytes() != B.x[i].tobytes(), who
        if u.tile is None:
            continue
        m = MT.inside(u.dims, u.tile)
        assert u.tile in MT.targets(u.dims, ty).values() and not B.x[i][~m].any() and B.x[i][m].all(), who
        assert all(o % (1 << u.L) == 0 and n % (1 << u.L) == 0 for o, n in u.tile), who
        # outside the tile every cell reconstructs to exactly 0 under any threshold ...
        for bb in (0, b, 4095):
            assert not MR.Unit(B.x[i], flat, u.L).recon(bb).reshape(m.shape)[~m].any(), (who, bb)
        # ... so a search that does not see the tile ends elsewhere
        blind = _Blind(B.x[i], flat, u.L, ~m)
        bb = MR.search(blind, B.E[i])
        assert (bb, blind.err(bb)) == (4095, 0.0) != (b, e), who
    names = {u.name.split("-", 2)[-1] for u in B.us if u.tile is not None}
    assert names == {"first", "last_x", "last_y", "last_z", "corner"}


@pytest.mark.parametrize("seed", SEEDS)
def test_leveltol_batches_through_the_host_rule(wc, oracle, seed):
    B = RF.leveltol_case(wc.capi, oracle, seed)
    some = deep = 0
    for i in range(B.n):
        W, H, D = B.dims[i]
        L, flat = B.levels[i], B.flat[i]
        pay, kept, th, bd = B.want[i]
        who = (seed, i, B.dims[i], L, B.tol[i])
        counts = LT.level_counts(flat, W, H, D, L) if flat.size else np.zeros((L, LT.HIST_BINS), np.uint64)
        gt, gb = wc.capi.tol_levels_threshold(counts, L, flat.size, B.tol[i])
        assert len(gt) == L and all(same_bits(gt[l], th[l], np.float32) for l in range(L)), (who, gt, th)
        assert same_bits(gb, bd) and gb <= B.tol[i], (who, gb, bd)
        with np.errstate(invalid="ignore"):
            live = int((np.abs(flat) > 0).sum())
        some += 0 < kept < live
        deep += B.stop[i] is not None and B.stop[i][1] > 1
    odd = sum(B.units[i].cell_offset % 2 and B.boxes[i].size > 0 for i in range(B.n))
    kinds = {"zero" if t == 0.0 else "inf" if t == np.inf else "finite" for t in B.tol}
    print(f"leveltol seed {seed}: n {B.n} keep some {some} stops past level 1 {deep} odd {odd}")
    assert some >= 3 and deep >= 1 and odd >= 8 and kinds == {"zero", "inf", "finite"}


@pytest.mark.parametrize("seed", SEEDS)
def test_pair_tolerance_batches_through_the_host_rule(wc, seed):
    before = [(u.payload, u.K, u.thresh.tobytes(), u.split, u.layers) for u in PF.batch(seed).us]
    T = PF.tol_batch(seed)
    assert [(u.payload, u.K, u.thresh.tobytes(), u.split, u.layers) for u in PF.batch(seed).us] == before
    some = none = drained = every = past = nan = 0
    for u, w, s in zip(T.us, T.want, T.split):
        who = (seed, u.name, u.dims, u.L, u.tol)
        assert TT.accepted(*u.dims, u.L), who
        out, th, bound = wc.capi.thin_tol_unit(u.payload, u.tol)
        same = TT.th_bits(th) == TT.th_bits(w[2], u.L) and TT.f64_bits(bound) == TT.f64_bits(w[3])
        assert out == w[0] and same, who
        base, rest, th, bound = wc.capi.split_tol_unit(u.payload, u.tol)
        same = TT.th_bits(th) == TT.th_bits(s[4], u.L) and TT.f64_bits(bound) == TT.f64_bits(s[5])
        assert base == s[0] == w[0] and rest == s[1] and same, who
        assert wc.capi.merge_unit(base, rest) == LR.canon(u.payload) == u.canon, who
        assert w[3] <= u.tol, who
        _, _, _, _, _, runs, bits = TR.parse(u.payload)
        livepos = LR.live_pairs(u.payload)[4]
        keepable = (len(u.canon) - 20) // 8  # what a zero tolerance keeps: the live pairs that are not +-0 or NaN
        some += 0 < w[1] < keepable
        none += w[1] == 0
        drained += w[1] == 0 < keepable
        every += w[1] == keepable > 0
        past += livepos.size < u.pairs
        nan += bool(((bits[:livepos.size] & np.uint32(0x7FFFFFFF)) > 0x7F800000).any())
    refused = [u for u in PF.batch(seed).us if u.tol is None]
    assert refused and all(not TT.accepted(*u.dims, u.L) and u.thin_tol is None for u in refused)
    kinds = {"zero" if t == 0.0 else "inf" if t == np.inf else "finite" for t in T.tol}
    print(f"pairs tol seed {seed}: accepted {T.n} of {PF.batch(seed).n} keep some {some} none {none} "
          f"(of pairs to keep: {drained}) all {every} past N {past} NaN {nan}")
    assert T.n >= 10 and some >= 5 and none >= 1 and every >= 1 and past >= 1 and nan >= 1
    assert kinds == {"zero", "inf", "finite"}
    assert max(-(-min(u.pairs, u.N) // TT.TILE) for u in T.us) >= 2  # both select paths at WC_OPT_TOL_SOLO_TILES = 1
