"""GPU: thinning, splitting and merging (include/wavelet_amd.h wc_thin_*, wc_split_*,
wc_merge and the _host forms) on units past the solo limit of the select and past
one window of the look-back, byte for byte against the numpy restatements
(thin_rule.py, layers_rule.py, budget_rule.py).  No tolerance anywhere.

The batch is pairs_scale.py's (test_pairs_scale_cpu.py proves what it holds): units
of 65, 68, 72 and 80 pair tiles beside one of exactly 64, so that under the default
options k_thin_digit / k_thin_pick run with chunk = 8 (whole chunks, a chunk of 4, a
chunk of 1, work items past the payload's pairs), lookback_sum slides past its
window of 64 tiles in ThinScan and in CountScan with Granule62 (and derives up to
79 predecessors under the forced-derive option sets), and both counts of a split
pass 2^16.  One K per class of budget_rule.classes() per unit, spread over the
calls of the batch.  The checks are test_gpu_thin.Dev.check, test_gpu_layers.
SplitDev.check and MergeDev.check unchanged: sentinels around every slot, no byte
outside a unit's payload written, the inputs untouched.  Every leg compares against
the same reference bytes, so the legs are identical to each other.

Then: merges whose bounded search spans 70 tiles of the other side or jumps a whole
block of 4097 ranks inside a tile; overlaps among good units; the device identity
merge(split(P)) == P with wc_inverse_levels of both; the host forms with every large
unit in a run of its own; and the forward modes' split select on a unit of 68
tiles, whose last chunk is partial (k_budget_split, k_budget_digit, k_ltol_split,
k_tol_split)."""
import numpy as np
import pytest

import budget_rule as BR
import decode_payloads as DP
import layers_rule as LR
import leveltol_rule as LT
import pairs_scale as PS
from pairs_scale import SOLO
from test_gpu_budget import Dev as BudgetDev
from test_gpu_fuzz import _OPTION_SETS
from test_gpu_layers import MergeDev, SplitDev
from test_gpu_leveltol import Dev as LevelTolDev
from test_gpu_modes_fuzz import LOOKBACK, options
from test_gpu_thin import Dev as ThinDev
from tol_rule import same_bits, tol_rule
from wavelet_compression_amd.capi import WC_MAX_LEVELS, WC_OPT_HOST_CHUNK, WC_OPT_TOL_SOLO_TILES

pytestmark = pytest.mark.gpu

LEGS = {"default": (), "solo_1": ((WC_OPT_TOL_SOLO_TILES, 1),), "solo_1000": ((WC_OPT_TOL_SOLO_TILES, 1000),)}
LEGS.update({o: _OPTION_SETS[o] for o in LOOKBACK})


def _run(wc, ctx, V, form, budget, what):
    if form == "thin":
        d = ThinDev(wc, V, budget)
        d.run(ctx)
        ctx.synchronize()
        d.check(what)
    else:
        d = SplitDev(wc, V, budget)
        d.run(ctx)
        ctx.synchronize()
        d.check(V.split, what)


@pytest.mark.parametrize("form", ["thin", "split"])
@pytest.mark.parametrize("leg", list(LEGS))
def test_budget_forms_on_the_large_batch(wc, ctx, leg, form):
    S = PS.scale(wc)
    large = [u.tiles for u in S.us if u.tiles > SOLO]
    if leg == "default":  # the select of every large unit is split over workgroups, in chunks of 8 tiles
        assert ctx.get_option(WC_OPT_TOL_SOLO_TILES) == SOLO < min(large) and SOLO in [u.tiles for u in S.us]
        assert {t % 8 for t in large} >= {0, 1, 4}
    with options(wc, ctx, LEGS[leg]):
        for j, V in enumerate(S.budget):
            _run(wc, ctx, V, form, True, (leg, form, "call", j))


@pytest.mark.parametrize("form", ["thin", "split"])
@pytest.mark.parametrize("leg", ["default", *LOOKBACK])
def test_threshold_forms_on_the_large_batch(wc, ctx, leg, form):
    S = PS.scale(wc)
    with options(wc, ctx, LEGS[leg]):
        for j, V in enumerate(S.thresh):
            _run(wc, ctx, V, form, False, (leg, form, "thresholds", j))


@pytest.mark.parametrize("leg", ["default", *LOOKBACK])
def test_merge_of_the_large_pairs_in_both_orders(wc, ctx, leg):
    M = PS.merge_case(wc)
    with options(wc, ctx, LEGS[leg]):
        for swap in (False, True):
            d = MergeDev(wc, M, one_buffer=swap)
            d.run(ctx, swap=swap)
            ctx.synchronize()
            d.check((leg, "b, a" if swap else "a, b"))


@pytest.mark.parametrize("leg", ["default", "tickets", "reversed_spin_1"])
def test_merge_overlaps_among_the_large_pairs(wc, ctx, leg):
    M = PS.merge_case(wc)
    abuf, aoff, bbuf, boff, ov, _, _ = PS.overlaps(M)
    S = type("Shadow", (), dict(vars(M), abuf=abuf, aoff=aoff, bbuf=bbuf, boff=boff))()
    with options(wc, ctx, LEGS[leg]):
        d = MergeDev(wc, S)
        d.run(ctx)
        with pytest.raises(wc.WaveletError) as ei:
            ctx.synchronize()
        assert ei.value.code == wc.capi.WC_ERR_FORMAT
        d.check(("overlaps", leg), overlap=ov)
        ctx.synchronize()  # the error word is cleared


def test_device_identity_on_the_field_payloads(wc, ctx):
    """wc_merge(wc_split_budget(P, c // 2)) == P on the five field payloads, and wc_inverse_levels of the merged
    payloads bit-equal to that of P; enqueued without a sync in between."""
    import torch
    S = PS.scale(wc)
    us = [u for u in S.us if u.kind == "field"]
    n = len(us)
    dims, levels = [u.dims for u in us], [u.L for u in us]
    K = [u.pairs // 2 for u in us]  # a field payload holds candidates alone: c = its pair count
    units, _, extent = wc.capi.make_units(dims)
    buf, off = DP.payload_layout([u.payload for u in us], np.random.default_rng(9505))
    dev = torch.device("cuda", 0)
    cap = wc.capi.payload_bound(units, n)
    bcap, rcap = wc.capi.split_bound(units, n, K)

    def bufs(c):
        return (torch.full((c,), 0xA5, dtype=torch.uint8, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev),
                torch.zeros(n, dtype=torch.int32, device=dev))

    P = (torch.from_numpy(buf).to(dev), torch.from_numpy(off.view(np.int64)).to(dev))
    base, rest, merged = bufs(bcap), bufs(rcap), bufs(cap)
    back_p = torch.full((extent,), -77.0, dtype=torch.float32, device=dev)
    back_m = torch.full((extent,), -78.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.split_budget(P[0].data_ptr(), P[1].data_ptr(), units, n, levels, K, base[0].data_ptr(), bcap, base[1].data_ptr(),
                     base[2].data_ptr(), rest[0].data_ptr(), rcap, rest[1].data_ptr(), rest[2].data_ptr())
    ctx.merge(rest[0].data_ptr(), rest[1].data_ptr(), base[0].data_ptr(), base[1].data_ptr(), units, n, levels,
              merged[0].data_ptr(), cap, merged[1].data_ptr(), merged[2].data_ptr())
    ctx.inverse_levels(merged[0].data_ptr(), merged[1].data_ptr(), units, n, levels, back_m.data_ptr())
    ctx.inverse_levels(P[0].data_ptr(), P[1].data_ptr(), units, n, levels, back_p.data_ptr())
    ctx.synchronize()

    def read(b):
        pay, o, cnt = b[0].cpu().numpy(), b[1].cpu().numpy().view(np.uint64), b[2].cpu().numpy().view(np.uint32)
        return [wc.capi.unit_payload(pay, o, cnt, i) for i in range(n)]

    got_b, got_r, got_m = read(base), read(rest), read(merged)
    for i, u in enumerate(us):
        want = LR.split_budget(u.payload, K[i])
        assert (got_b[i], got_r[i]) == want[:2] and 20 < len(got_b[i]) < len(u.payload), u.name
        assert got_m[i] == u.payload, u.name
    assert back_m.cpu().numpy().tobytes() == back_p.cpu().numpy().tobytes()
    owned = np.zeros(extent, bool)
    for i, u in enumerate(us):
        owned[units[i].cell_offset:units[i].cell_offset + u.N] = True
    assert not (back_p.cpu().numpy()[owned] == -77.0).any()


def test_host_forms_with_every_large_unit_in_a_run_of_its_own(wc, ctx):
    S = PS.scale(wc)
    V = S.budget[0]
    M = PS.merge_case(wc)

    def packed(out, off, cnt, exp, what):
        o = 4  # packed as wc_forward_host: 24 + 8 pairs bytes apart, from 4
        for i, w in enumerate(exp):
            assert int(off[i]) == o and 20 + 8 * int(cnt[i]) == len(w), (what, i)
            assert out[o:o + len(w)].tobytes() == w, (what, i)
            o += len(w) + (4 if i + 1 < len(exp) else 0)
        assert int(off[len(exp)]) == o, what

    with options(wc, ctx, ((WC_OPT_HOST_CHUNK, 1 << 18),)):
        assert all(u.N > 1 << 18 for u in S.us if u.tiles > SOLO) and all(p.N > 1 << 18 for p in M.ps)
        base, boff, kept, rest, roff, rpairs, th, key = ctx.split_host(S.buf, S.off, S.units, S.n, S.levels, max_pairs=V.K)
        packed(base, boff, kept, [w[0] for w in V.split], "base")
        packed(rest, roff, rpairs, [w[1] for w in V.split], "rest")
        for i, u in enumerate(S.us):
            assert int(key[i]) == V.split[i][4] and all(
                same_bits(float(th[i, l]), V.split[i][5][l] if l < u.L else 0.0, np.float32)
                for l in range(WC_MAX_LEVELS)), (i, u.name)
        out, off, pairs = ctx.merge_host(rest, roff, base, boff, S.units, S.n, S.levels)
        packed(out, off, pairs, [LR.canon(u.payload) for u in S.us], "merged")
        out, off, pairs = ctx.merge_host(M.abuf, M.aoff, M.bbuf, M.boff, M.units, M.n, None)
        packed(out, off, pairs, M.want, "merge batch")


def test_forward_selects_split_a_unit_of_68_tiles(wc, ctx, oracle):
    """The forward modes' split select with a partial last chunk (68 = 8 * 8 + 4 tiles) under the default
    options: wc_forward_levels_budget and wc_forward_levels_tol at L = 2, wc_forward_tol at L = 1, against
    budget_rule.payload, leveltol_rule.payload and tol_rule as their own tests compare."""
    dims, L = PS.BOX68, 2
    box = PS.field_box(2)
    assert box.shape == dims[::-1] and PS.plan_tiles(dims) == 68 > ctx.get_option(WC_OPT_TOL_SOLO_TILES) == SOLO
    units, n, _ = wc.capi.make_units([dims])
    cells = box.ravel().copy()
    # the budget mode
    prep = BR.prepare(box, L)
    K = len(prep[7]) // 3
    pay, kept, T, th, _ = BR.payload_of(prep, K)
    d = BudgetDev(wc, units, n, cells)
    ctx.forward_levels_budget(d.cells.data_ptr(), d.code, units, n, [L], [K], *d.out_args())
    ctx.synchronize()
    pays, gk, off, gth, key = d.read()
    assert pays[0] == pay and int(gk[0]) == kept <= K and int(key[0]) == T and int(off[0]) == 4
    assert all(same_bits(float(gth[0, l]), th[l] if l < L else 0.0, np.float32) for l in range(WC_MAX_LEVELS))
    # the per-level tolerance
    tol = 10.0 ** -1.5 * float(np.sqrt(np.mean(box.astype(np.float64) ** 2)))
    pay, kept, th, bd, _, _ = LT.payload(box, L, tol)
    d = LevelTolDev(wc, None, units, n, cells)
    ctx.forward_levels_tol(d.cells.data_ptr(), d.code, units, n, [L], [tol], *d.out_args())
    ctx.synchronize()
    pays, gk, off, gth, bound = d.read()
    assert pays[0] == pay and int(gk[0]) == kept and 0 < kept < box.size and same_bits(float(bound[0]), bd)
    assert all(same_bits(float(gth[0, l]), th[l] if l < L else 0.0, np.float32) for l in range(WC_MAX_LEVELS))
    # the one-level tolerance
    flat = oracle.wavelet_decompose(box)
    t, bd = tol_rule(oracle.magnitude_hist(flat), flat.size, tol)
    pay = oracle.compress_payload_thresh(box, t)
    d = LevelTolDev(wc, None, units, n, cells)
    ctx.forward_tol(d.cells.data_ptr(), d.code, units, n, [tol], d.pay.data_ptr(), d.cap, d.off.data_ptr(),
                    d.kept.data_ptr(), d.thresh.data_ptr(), d.bound.data_ptr())
    ctx.synchronize()
    pays, gk, off, gth, bound = d.read()
    assert pays[0] == pay and 0 < int(gk[0]) < box.size
    assert same_bits(float(gth.ravel()[0]), t, np.float32) and same_bits(float(bound[0]), bd)
