"""The large batch of the pair pipeline (pairs_scale.py) and the seeded random
batches (pairs_fuzz.py) without a GPU: the batches show what they claim, proved from
the numpy restatements alone (thin_rule.py, layers_rule.py, budget_rule.py), and the
host rule (wc_thin_unit, wc_split_unit, wc_merge_unit) equals the restatement byte
for byte on every unit and every K of them."""
import numpy as np

import budget_rule as BR
import layers_rule as LR
import pairs_fuzz as PF
import pairs_scale as PS
import thin_rule as TR
from pairs_scale import SOLO, TILE
from tol_rule import same_bits


def test_the_large_batch_shows_what_it_claims(wc):
    S = PS.scale(wc)
    by = {u.name: i for i, u in enumerate(S.us)}
    fields = [u for u in S.us if u.kind == "field"]
    assert [u.tiles for u in fields] == [65, 72, 68, 80, 64] and [u.L for u in fields] == [1, 3, 2, 4, 4]
    assert all(u.N == u.tiles * TILE for u in fields)  # whole tiles: 65 exactly, one past the solo limit
    assert all(LR.canon(u.payload) == u.payload and u.pairs > u.N // 2 for u in fields)
    assert S.calls == max(len(a) for a in S.avail) >= 14  # as many calls as the largest class set needs
    # every class of budget_rule.classes() on a unit that the default options split, and on one they do not
    for cl in BR.CLASSES + PS.EXTRA:
        tiles = {S.us[i].tiles for _, i in S.where(cl)}
        assert any(t > SOLO for t in tiles) and any(t <= SOLO for t in tiles), (cl, sorted(tiles))
    for u, a in zip(S.us, S.avail):  # a field payload shows every class its L admits, bar the two of special values
        if u.kind == "field":
            missing = set(BR.CLASSES) - set(a)
            assert missing <= {"inf", "last_zero"} | ({"cross_level"} if u.L == 1 else set()), (u.name, missing)
    assert "last_zero" in S.avail[by["tiny"]] and "inf" in S.avail[by["inf"]]
    # what a class means, on every (call, unit) that shows it
    for j, V in enumerate(S.budget):
        for i, u in enumerate(S.us):
            cl, K = S.shown[j][i], V.K[i]
            base, rest, kept, rpairs, T, th = V.split[i]
            c = S.avail[i]["all"]
            who = (j, u.name, cl, K)
            assert kept <= min(K, c) and kept + rpairs == c, who
            assert (len(base), len(rest)) == (20 + 8 * kept, 20 + 8 * rpairs), who
            if cl == "tie":
                assert kept < K < c, who
            if cl in ("all", "over"):
                assert T == 0 and rpairs == 0 and base == LR.canon(u.payload), who
            if cl == "zero":
                assert kept == 0 and rest == LR.canon(u.payload), who
            if cl == "low_00":
                assert T & 0x7F == 0 and T, who
            if cl == "low_7f":
                assert T & 0x7F == 0x7F, who
            if cl == "mid_000":
                assert (T >> 7) & 0xFFF == 0 and T, who
            if cl == "mid_fff":
                assert (T >> 7) & 0xFFF == 0xFFF, who
            if cl == "inf":
                assert th[0] == np.inf, who
            if cl == "last_zero":
                assert th[-1] == 0.0 and th[0] > 0.0 and u.L >= 2, who
            if cl == "half" and u.name in ("field-72", "field-80"):
                assert kept > 65536 and rpairs > 65536, who  # both counts of the split past 16 bits
            if cl == "hundred" and u.kind == "field":
                assert 0 < kept <= 100 < 65536 < rpairs, who  # a base under a tile, a rest past 16 bits
    for n in ("field-72", "field-80"):
        assert any(i == by[n] for _, i in S.where("half")) and any(i == by[n] for _, i in S.where("hundred")), n
    # the crafted unit: a pair at every position, every exponent, the specials, a tie of 5000
    u = S.us[by["every-position"]]
    _, _, _, _, _, runs, bits = TR.parse(u.payload)
    m = bits & np.uint32(0x7FFFFFFF)
    assert u.tiles == 65 and runs.size == u.N and not runs.any()
    assert set((m >> 23).tolist()) == set(range(256)) and set(PS.SPECIALS.tolist()) <= set(bits.tolist())
    assert int((m == np.float32(3.25).view(np.uint32)).sum()) == PS.TIE
    assert len(np.unique(BR.keys(bits.view(np.float32), *u.dims, 1)[0] >> 19)) > 3000  # first-digit bins in use
    assert {"tie", "inf"} <= set(S.avail[by["every-position"]])
    # the sparse units: fewer pair tiles than plan tiles, the pair count at a chunk of 8 tiles and +-1
    sparse = [u for u in S.us if u.kind == "sparse"]
    assert [u.pairs for u in sparse] == [8 * TILE - 1, 8 * TILE, 8 * TILE + 1, 9 * TILE + 1]
    assert sorted(u.L for u in sparse) == [1, 2, 3, 4]
    for u in sparse:
        assert LR.live_pairs(u.payload)[4].size == u.pairs  # all below N: np is the pair count
        assert -(-u.pairs // TILE) in (8, 9, 10) and u.tiles == 80 > SOLO  # whole work items hold no pair
    assert any("last_zero" in S.avail[by[u.name]] for u in sparse)
    assert (S.us[by["n=0"]].pairs, S.us[by["n=1"]].pairs) == (0, 1) and S.us[by["n=0"]].tiles == 72
    # the surplus unit: a tile and one pair past N; min(pair tiles, plan tiles) = all 68
    u = S.us[by["surplus"]]
    assert u.pairs == u.N + TILE + 1 and min(-(-u.pairs // TILE), u.tiles) == u.tiles == 68
    assert LR.live_pairs(u.payload)[4].size == u.N
    # the thresholds: per level a magnitude that occurs there (the strict > decides), 0.0, +inf on one level
    occ, zero, inf = S.thresh
    assert not zero.thresh.any()
    for i, u in enumerate(S.us):
        for l in range(u.L):
            a = S.occurring[i][l]
            assert (occ.thresh[i, l] in a) if a.size else occ.thresh[i, l] == 0.0, (u.name, l)
        assert int(np.isinf(inf.thresh[i]).sum()) == 1, u.name
        if u.kind == "field":
            assert 0 < occ.split[i][2] < u.pairs and inf.split[i][2] < occ.split[i][2], u.name
            assert (inf.split[i][2] > 0) == (u.L > 1), u.name  # L = 1: +inf on its one level keeps nothing
            assert zero.split[i][0] == u.payload and zero.split[i][3] == 0, u.name


def test_the_host_rule_equals_the_restatement_on_the_large_batch(wc):
    capi = wc.capi
    S = PS.scale(wc)
    for j, V in enumerate(S.budget + S.thresh):
        budget = j < S.calls
        for i, u in enumerate(S.us):
            who = (j, u.name, V.K[i])
            wbase, wrest = V.split[i][:2]
            kw = dict(max_pairs=V.K[i]) if budget else dict(thresh=V.thresh[i, :u.L])
            base, rest, T, th = capi.split_unit(u.payload, **kw)
            assert (base, rest) == (wbase, wrest), who
            assert capi.thin_unit(u.payload, **kw)[0] == wbase, who
            if budget:
                assert T == V.split[i][4], who
                assert all(same_bits(float(a), b, np.float32) for a, b in zip(th, V.split[i][5])), who
            assert capi.merge_unit(base, rest) == capi.merge_unit(rest, base) == LR.canon(u.payload), who


def test_the_merge_pairs_show_what_they_claim_and_the_host_rule_merges_them(wc):
    M = PS.merge_case(wc)
    by = {p.name: i for i, p in enumerate(M.ps)}
    assert [PS.plan_tiles(p.dims) for p in M.ps] == [72, 72, 80, 68, 65, 68, 72]
    pos = [(LR.live_pairs(p.pay[0])[4], LR.live_pairs(p.pay[1])[4]) for p in M.ps]
    for p, (a, b), w in zip(M.ps, pos, M.want):
        assert (a.size, b.size) == p.live and np.intersect1d(a, b).size == 0, p.name
        assert wc.capi.merge_unit(p.pay[0], p.pay[1]) == wc.capi.merge_unit(p.pay[1], p.pay[0]) == w, p.name
        assert len(w) == 20 + 8 * (a.size + b.size), p.name

    def spans(mine, other):
        """Per tile of `mine`: the entries of `other` between its first and last position."""
        return [int(np.searchsorted(other, mine[min(k + TILE, mine.size) - 1]) - np.searchsorted(other, mine[k]))
                for k in range(0, mine.size, TILE)]

    a, b = pos[by["a:alternating"]]
    assert a.size == b.size == 147456 and not TR.parse(M.want[by["a:alternating"]])[5].any()
    a, b = pos[by["b:every-71st"]]
    assert TILE < a.size <= 2 * TILE and a.size + b.size == 72 * TILE
    assert spans(a, b)[0] >= 60 * TILE and a[-1] > 71 * TILE  # a's first tile spans 60 tiles of b and more
    a, b = pos[by["c:a-before-b"]]
    assert (a[0], a[-1], b[0], b[-1]) == (0, 199999, 200000, 80 * TILE - 1)
    a, b = pos[by["d:blocks-4097"]]
    sa, sb = spans(a, b), spans(b, a)
    # every tile but a side's first and last: a rank jump of a whole block inside it
    assert len(sa) >= 30 and all(s >= TILE + 1 for s in sa[1:-1] + sb[1:-1]), (sa, sb)
    a, b = pos[by["e:one-to-three"]]
    assert a.size + b.size == 65 * TILE and 0.24 < a.size / (65 * TILE) < 0.26
    p = M.ps[by["f:past-N"]]
    a, b = pos[by["f:past-N"]]
    assert a.size + b.size == p.N and ((len(p.pay[0]) - 20) // 8, (len(p.pay[1]) - 20) // 8) == (a.size + 5000, b.size + 70)
    a, b = pos[by["g:b-empty"]]
    assert a.size == 147456 and b.size == 0 and len(M.ps[by["g:b-empty"]].pay[1]) == 20
    bits = np.concatenate([TR.parse(w)[6] for w in M.want])
    m = bits & 0x7FFFFFFF
    assert (m == 0).any() and (m > 0x7F800000).any() and (m == 0x7F800000).any() and ((m > 0) & (m < 0x00800000)).any()
    # the overlap units: one shared position each, refused by the rule
    abuf, aoff, bbuf, boff, ov, apays, bpays = PS.overlaps(M)
    for i in range(M.n):
        a, b = LR.live_pairs(apays[i])[4], LR.live_pairs(bpays[i])[4]
        shared = np.intersect1d(a, b)
        if i not in ov:
            assert (apays[i], bpays[i]) == tuple(M.ps[i].pay) and shared.size == 0
            continue
        assert shared.tolist() == ([72 * TILE - 2] if M.ps[i].name == "a:alternating" else [200000]), M.ps[i].name
        for x, y in ((apays[i], bpays[i]), (bpays[i], apays[i])):
            try:
                wc.capi.merge_unit(x, y)
                raise AssertionError("merged an overlap")
            except wc.WaveletError as e:
                assert e.code == wc.capi.WC_ERR_FORMAT


def test_the_fuzz_batches_through_the_host_rule(wc):
    """Seeds 0 and 1 of pairs_fuzz.batch(): the generator's claims, and every check of test_gpu_pairs_fuzz.py on
    the host rule, which pins the generator and the restatement to each other."""
    capi = wc.capi
    counts, kinds = set(), set()
    for seed in (0, 1):
        B = PF.batch(seed)
        assert 20 <= B.n <= 28 and sum(PS.plan_tiles(u.dims) > SOLO for u in B.us) == 1
        assert any(u.N == 0 for u in B.us) and any((u.dims[0] | u.dims[1] | u.dims[2]) & 1 for u in B.us)
        assert all(u.N <= 1 << 15 or 65 <= PS.plan_tiles(u.dims) <= 70 for u in B.us)
        for i, u in enumerate(B.us):
            who = (seed, i, u.name)
            _, _, _, _, _, runs, bits = TR.parse(u.payload)
            assert runs.size == 0 or int(runs.max()) <= 2 ** 31 - 1, who
            counts.add(u.pairs)
            kinds |= {"overshoot"} if u.pairs <= u.N and LR.live_pairs(u.payload)[4].size < u.pairs else set()
            kinds |= {"surplus"} if u.pairs > u.N else set()
            kinds |= {"layer-past-N"} if any((len(l) - 20) // 8 > LR.live_pairs(l)[4].size for l in u.layers) else set()
            kinds |= {"three-layers"} if len(u.layers[2]) > 20 else set()
            base, rest, T, th = capi.split_unit(u.payload, max_pairs=u.K)
            assert (base, rest, T) == (u.split[0], u.split[1], u.split[4]), who
            assert capi.thin_unit(u.payload, max_pairs=u.K)[0] == u.split[0], who
            assert capi.split_unit(u.payload, thresh=u.thresh[:u.L])[:2] == u.tsplit[:2], who
            assert capi.thin_unit(u.payload, thresh=u.thresh[:u.L])[0] == u.tsplit[0], who
            b2, r2, _, _ = capi.split_unit(rest, max_pairs=u.K2)
            assert (b2, r2) == u.split2[:2], who
            assert capi.merge_unit(base, capi.merge_unit(b2, r2)) == u.canon == LR.canon(u.payload), who
            l0, l1, l2 = u.layers
            left = capi.merge_unit(capi.merge_unit(l0, l1), l2)
            right = capi.merge_unit(l0, capi.merge_unit(l1, l2))
            assert left == right == u.merged, who
            assert capi.merge_unit(l0, l1) == capi.merge_unit(l1, l0) == u.merged01, who
    assert counts >= set(PF.COUNTS), sorted(counts)
    assert kinds == {"overshoot", "surplus", "layer-past-N", "three-layers"}, kinds
