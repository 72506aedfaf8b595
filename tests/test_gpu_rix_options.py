"""The row-indexed inverse (wc_inverse.hip k_rowindex + k_inverse_rows, "K6r")
under every tile shape and tile order its options can produce, against the CPU
oracle.

include/wavelet_amd.h promises "Same cells" for WC_OPT_RIX_LDS (the workgroup's
LDS budget, from which the plan derives the tile TX x TY), WC_OPT_RIX_TX (upper
bound on log2 TX), WC_OPT_RIX_BLOCKED (contiguous tile runs per workgroup),
WC_OPT_RIX_XCD (the tile list permuted over the XCDs, one unit group) and
WC_OPT_INV_GROUPS; with the defaults a unit only ever sees one tile shape.  The
batch below is chosen so that the cross of the options reaches the kernel
branches the defaults leave alone:

  * TX = 32: a wave owns twice the 16 prefetch slots, ranges j >= NR are loaded
    when scattered (NR 16, 13 or 7 with the forms of the fused RMSE);
  * TX = 1: x-pair stores and the separate RMSE pass on a 16-B-aligned output;
  * edge tiles in x (W/2 no multiple of TX) and y (H/2 no multiple of TY), with
    x-quad and with x-pair stores;
  * ranges of more than one 64-pair round (keep 1.0: every coefficient kept);
  * the budget fallback: a fast-shape unit whose one-block tile (4 D + 80
    floats) exceeds the budget decodes densely beside row-indexed ones, so
    wc_inverse_rmse takes its two-call path and wc_inverse_rows ignores row
    entries the forward wrote;
  * blocked tile runs, the XCD permutation (the fused RMSE's partial sums stay
    in unit order), unit groups;
  * the largest tile: 64 x 2 x 120 at budget 16384, RIX_TX 5 needs 63 744 B of
    dynamic LDS.

One generic unit in a batch sends wc_inverse_rmse through its two-call path
(wc_inverse + wc_rmse), so the batch runs twice: "mixed", with its generic
units, and "fast", with fast-shape units of about their size in their place,
where every unit with cells is row-indexed and the RMSE is fused into K6r (the
x-quad synthesis' own sums, the separate pass, the partial-sum slots in unit
order under the XCD permutation).

tests/cpp/test_plan.cpp bounds the kernel's addresses for these same units and
option sets on the CPU.  Here, per option set, wc_inverse, wc_inverse_rows (the
forward's row index) and wc_inverse_rmse (fp64 originals at a 16-B-aligned
base, 8 bytes past one, fp32 originals) each write buffers pre-filled with a
sentinel: every unit's cells equal the oracle's decompress() bit for bit
(test_gpu_fuzz.same_cells), every cell outside the units keeps the sentinel,
every RMSE is within the suite's summation-order bound of calc_rmse_per_box
(max(1e-12, (n + 4) 2^-53) relative, tests/test_gpu_fuzz.py).
"""
import numpy as np
import pytest

from test_gpu_fuzz import same_cells
from wavelet_compression_amd.capi import (WC_ERR_INVALID, WC_OPT_INV_GROUPS, WC_OPT_RIX_BLOCKED, WC_OPT_RIX_LDS,
                                          WC_OPT_RIX_TX, WC_OPT_RIX_XCD, WaveletError)

pytestmark = pytest.mark.gpu

# (W, H, D); tests/cpp/test_plan.cpp has the same list and offsets
DIMS = [
    (5, 4, 8),      # generic (odd W)
    (64, 2, 8),     # TX reaches 32, a single y block
    (66, 6, 8),     # hx 33, hy 3: edge tiles in both axes; W % 4 == 2: x-pair stores
    (6, 6, 4),      # generic (D % 8 != 0)
    (72, 10, 16),   # hx 36, W % 4 == 0: x-quad stores with a 4-block edge tile; hy 5
    (64, 2, 120),   # 120 pairs per range; TX 32 at 16384: 63 744 B of LDS
    (32, 32, 32),   # a cube at an odd offset: scalar stores
    (64, 8, 24),    # TY 4 at 16384, 2 at 9216 (RIX_TX 5)
    (8, 64, 8),     # tall in y, TY up to 32; offset == 2 (mod 4): 8-B stores
    (0, 4, 8),      # empty
    (2, 2, 232),    # the fallback boundary at 1024: row-indexed
    (2, 2, 240),    # ... and dense
    (16, 16, 64),   # a cube
    (32, 4, 8),     # all zero
    (64, 2, 16),    # a single pair at the last flat position
]
ZERO_UNIT, LAST_PAIR_UNIT = 13, 14
# the "fast" batch: the generic units 0 and 3 replaced, so that the fused RMSE runs
FAST_DIMS = [(4, 4, 8) if i == 0 else (6, 6, 8) if i == 3 else d for i, d in enumerate(DIMS)]
BATCH_DIMS = {"mixed": DIMS, "fast": FAST_DIMS}
KEEPS = (float(np.float32(1.0)), float(np.float32(0.999)))
BUDGETS = (1024, 2048, 9216, 16384)
SENTINEL = 0xC2F7A5A5  # a finite float32 (about -123.8) no reconstruction of these fields produces
# WC_OPT_INV_GROUPS 3 (without XCD) at two points of the cross: (budget, RIX_TX, BLOCKED)
GROUP_POINTS = {9216: (4, 0), 2048: (5, 1)}


def _offsets(dims):
    """Gaps of whole x-quads; every third unit one element past a quad, unit 8 two past."""
    offs, cur = [], 0
    for i, (W, H, D) in enumerate(dims):
        cur += 4 * ((i * 3) % 5)
        cur = (cur + 3) & ~3
        if i % 3 == 0:
            cur += 1
        elif i == 8:
            cur += 2
        offs.append(cur)
        cur += W * H * D
    return offs, cur


def _fields(oracle, flip, dims):
    """The smooth field and a Gaussian, alternating (the other way round at the second keep)."""
    rng = np.random.default_rng(77 + flip)
    boxes = []
    for i, (W, H, D) in enumerate(dims):
        if i == ZERO_UNIT:
            b = np.zeros((D, H, W))
        elif i == LAST_PAIR_UNIT:  # the last 2x2x2 block alternates in sign: only its x, y, z difference is non-zero
            b = np.zeros((D, H, W))
            s = np.array([1.0, -1.0])
            b[-2:, -2:, -2:] = 3.0 * s[:, None, None] * s[None, :, None] * s[None, None, :]
        elif (i + flip) % 2 == 0:
            b = oracle.synth_box_f64(oracle.unit_seed(7, 2, i, flip), (3 * i, 5 * i, 7 * i), W, H, D)
        else:
            b = rng.standard_normal((D, H, W)) * 100.0
        boxes.append(np.ascontiguousarray(b, np.float64))
    return boxes


_BATCHES = {}


def _batch(wc, ctx, oracle, which, ki):
    """Once per batch and keep: the forward (payloads + row index, checked
    against the oracle's), the oracle's reconstructions and RMSEs, the device
    buffers."""
    if (which, ki) in _BATCHES:
        return _BATCHES[which, ki]
    import torch
    keep = KEEPS[ki]
    dev = torch.device("cuda", 0)
    dims = BATCH_DIMS[which]
    boxes = _fields(oracle, ki, dims)
    offs, extent = _offsets(dims)
    units, n, ext = wc.capi.make_units(dims, offsets=offs)
    assert ext == extent and offs[8] % 4 == 2 and all(offs[i] % 2 == 1 for i in range(0, n, 3))
    total = (extent + 8 + 3) & ~3  # sentinels after the last unit too; rows of the stacked outputs stay 16-B aligned
    host = np.zeros(total, np.float64)
    host32 = np.zeros(total, np.float32)
    want = np.full(total, SENTINEL, np.uint32).view(np.float32)
    inside = np.zeros(total, bool)
    ref_rmse = np.zeros(n)
    payloads = []
    for i, b in enumerate(boxes):
        o = offs[i]
        b32 = oracle.narrow(b)
        host[o:o + b.size] = b.ravel()
        host32[o:o + b.size] = b32.ravel()
        p, k = oracle.compress_payload(b32, keep)
        payloads.append((p, k))
        if b.size:
            back = oracle.decompress_payload(p)
            want[o:o + b.size] = back.ravel()
            inside[o:o + b.size] = True
            ref_rmse[i] = oracle.rmse(b32, back)
    # the special units are what they are meant to be
    assert payloads[ZERO_UNIT][1] == 0
    _, nc, runs, _ = oracle.parse_payload(payloads[LAST_PAIR_UNIT][0])
    assert payloads[LAST_PAIR_UNIT][1] == 1 and int(runs[0]) == nc - 1
    if ki == 0:  # keep 1.0 keeps every non-zero coefficient: ranges of more than one 64-pair round
        assert payloads[5][1] > 0.9 * boxes[5].size

    cells = torch.from_numpy(host).to(dev)
    shifted = torch.zeros(total + 1, dtype=torch.float64, device=dev)
    shifted[1:] = cells
    cells32 = torch.from_numpy(host32).to(dev)
    assert cells.data_ptr() % 16 == 0 and shifted[1:].data_ptr() % 16 == 8
    cap = wc.capi.payload_bound(units, n)
    rb = wc.capi.rowindex_bytes(units, n)
    pay = torch.zeros(cap, dtype=torch.uint8, device=dev)
    po = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    kept = torch.zeros(n, dtype=torch.int32, device=dev)
    rows = torch.zeros(rb // 8, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.forward_rows(cells.data_ptr(), wc.capi.WC_F64, units, n, keep, pay.data_ptr(), cap, po.data_ptr(),
                     kept.data_ptr(), rows.data_ptr(), rb)
    ctx.synchronize()
    P, O_, K = pay.cpu().numpy(), po.cpu().numpy(), kept.cpu().numpy()
    for i, (p, k) in enumerate(payloads):
        a = int(O_[i])
        assert P[a:a + 20 + 8 * int(K[i])].tobytes() == p and int(K[i]) == k, (which, i, dims[i], keep)
    B = dict(which=which, dims=dims, units=units, n=n, offs=offs, total=total, want=want, inside=inside, ref_rmse=ref_rmse, cells=cells,
             shifted=shifted, cells32=cells32, pay=pay, po=po, rows=rows, rb=rb,
             out=torch.zeros((5, total), dtype=torch.float32, device=dev),
             rmse=torch.zeros((3, n), dtype=torch.float64, device=dev))
    _BATCHES[which, ki] = B
    return B


CALLS = ("wc_inverse", "wc_inverse_rows", "wc_inverse_rmse fp64 aligned", "wc_inverse_rmse fp64 + 8 B",
         "wc_inverse_rmse fp32")


def _run_set(wc, ctx, B, opts):
    """The five calls under one option set; returns the failures as strings."""
    import torch
    names = {WC_OPT_RIX_LDS: "RIX_LDS", WC_OPT_RIX_TX: "RIX_TX", WC_OPT_RIX_BLOCKED: "BLOCKED", WC_OPT_RIX_XCD: "XCD",
             WC_OPT_INV_GROUPS: "INV_GROUPS"}
    tag = B["which"] + " batch, " + " ".join(f"{names[k]} {v}" for k, v in opts)
    units, n, out, rmse = B["units"], B["n"], B["out"], B["rmse"]
    # every output buffer re-filled: a call that writes nothing cannot pass on the previous set's cells
    out.view(torch.int32).fill_(SENTINEL - (1 << 32))
    rmse.fill_(-1.0)
    torch.cuda.synchronize()
    before = [(k, ctx.get_option(k)) for k, _ in opts]
    try:
        for k, v in opts:
            ctx.set_option(k, v)
        pay, po = B["pay"].data_ptr(), B["po"].data_ptr()
        ctx.inverse(pay, po, units, n, out[0].data_ptr())
        ctx.inverse_rows(pay, po, units, n, B["rows"].data_ptr(), out[1].data_ptr(), rowinfo_capacity=B["rb"])
        ctx.inverse_rmse(pay, po, units, n, B["cells"].data_ptr(), wc.capi.WC_F64, out[2].data_ptr(), rmse[0].data_ptr())
        ctx.inverse_rmse(pay, po, units, n, B["shifted"][1:].data_ptr(), wc.capi.WC_F64, out[3].data_ptr(),
                         rmse[1].data_ptr())
        ctx.inverse_rmse(pay, po, units, n, B["cells32"].data_ptr(), wc.capi.WC_F32, out[4].data_ptr(), rmse[2].data_ptr())
        ctx.synchronize()
    finally:
        for k, v in before:
            ctx.set_option(k, v)
    got, E = out.cpu().numpy(), rmse.cpu().numpy()
    want, inside, offs = B["want"], B["inside"], B["offs"]
    bad = []
    for c, call in enumerate(CALLS):
        if not same_cells(got[c], want):  # units and sentinels at once; on a mismatch, say where
            for i, (W, H, D) in enumerate(B["dims"]):
                o, sz = offs[i], W * H * D
                if sz and not same_cells(got[c][o:o + sz], want[o:o + sz]):
                    bad.append(f"{tag}: {call}: unit {i} {W} x {H} x {D} differs from the oracle's cells")
            g, w = got[c].view(np.uint32), want.view(np.uint32)
            hit = np.flatnonzero(~inside & (g != w))
            if hit.size:
                bad.append(f"{tag}: {call}: {hit.size} cells outside the units overwritten, first at element {hit[0]}")
    worst = 0.0  # largest relative RMSE deviation of the set (shown with -s or on failure)
    for r, call in enumerate(CALLS[2:]):
        for i, (W, H, D) in enumerate(B["dims"]):
            ref, e, sz = B["ref_rmse"][i], E[r][i], W * H * D
            if np.isnan(ref) or np.isinf(ref):
                ok = np.isnan(e) if np.isnan(ref) else e == ref
            else:
                ok = np.isfinite(e) and abs(e - ref) <= max(1e-12, (sz + 4) * 2.0 ** -53) * abs(ref)
                if ok and ref:
                    worst = max(worst, abs(e - ref) / abs(ref))
            if not ok:
                bad.append(f"{tag}: {call}: unit {i} {W} x {H} x {D} rmse {e!r}, oracle {ref!r}")
    print(f"{tag}: {len(bad)} failures, largest relative RMSE deviation {worst:.3g}")
    return bad


@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("ki", range(len(KEEPS)), ids=["keep1", "keep0.999"])
@pytest.mark.parametrize("which", sorted(BATCH_DIMS))
def test_rix_option_cross(wc, ctx, oracle, which, ki, budget):
    """RIX_TX 0..5 x BLOCKED x XCD at one budget and one keep (plus INV_GROUPS 3
    at GROUP_POINTS), on the mixed and on the fast-only batch: no unit and no
    option set skipped."""
    B = _batch(wc, ctx, oracle, which, ki)
    sets = [((WC_OPT_RIX_LDS, budget), (WC_OPT_RIX_TX, tx), (WC_OPT_RIX_BLOCKED, blocked), (WC_OPT_RIX_XCD, xcd))
            for tx in range(6) for blocked in (0, 1) for xcd in (0, 1)]
    if budget in GROUP_POINTS:
        tx, blocked = GROUP_POINTS[budget]
        sets.append(((WC_OPT_RIX_LDS, budget), (WC_OPT_RIX_TX, tx), (WC_OPT_RIX_BLOCKED, blocked), (WC_OPT_RIX_XCD, 0),
                     (WC_OPT_INV_GROUPS, 3)))
    bad = []
    for opts in sets:
        bad += _run_set(wc, ctx, B, opts)
    assert not bad, f"{len(bad)} failures over {len(sets)} option sets, {which} batch, keep {KEEPS[ki]}:\n" + "\n".join(bad[:40])


def test_rix_option_validation(wc, ctx):
    """wc_set_option refuses WC_OPT_RIX_LDS outside 1024..16384 and WC_OPT_RIX_TX
    outside 0..5 (WC_ERR_INVALID, the old value stays); the boundary values are
    accepted and read back."""
    for opt, refused, accepted in ((WC_OPT_RIX_LDS, (1023, 16385), (1024, 16384)), (WC_OPT_RIX_TX, (-1, 6), (0, 5))):
        before = ctx.get_option(opt)
        try:
            for v in refused:
                with pytest.raises(WaveletError) as e:
                    ctx.set_option(opt, v)
                assert e.value.code == WC_ERR_INVALID, (opt, v)
                assert ctx.get_option(opt) == before, (opt, v)
            for v in accepted:
                ctx.set_option(opt, v)
                assert ctx.get_option(opt) == v, (opt, v)
                for r in refused:
                    with pytest.raises(WaveletError):
                        ctx.set_option(opt, r)
                    assert ctx.get_option(opt) == v, (opt, v, r)
        finally:
            ctx.set_option(opt, before)
        assert ctx.get_option(opt) == before
