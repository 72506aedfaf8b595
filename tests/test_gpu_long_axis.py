"""GPU: units with one long axis (tests/long_axis_shapes.py: pencils, slabs and
lines of up to 4097 cells along x, y or z, three units of exactly 2^21 cells)
through every device and host entry point, against the CPU oracle and the
opt-in modes' CPU restatements.

The plan (csrc/wc_plan.cpp) chooses kernels and tile shapes from exactly what a
long axis moves: the row-index fallback 4 D + 80 <= WC_OPT_RIX_LDS and the
shrinking x extent of the row-indexed tile, the multiply form of the row
division (D no power of two), sparse staging with 32 z tiles per unit, the
transform's 32 x 1 x 32 form on one block row, the emit class at 2^21 cells,
the generic transform's tail-only last tile.  tests/test_long_axis_cpu.py proves
that the list holds those classes; tests/cpp/test_plan.cpp checks the plan of
the same units on the CPU.  Here the kernels run.

One convention for every comparison.  Payload bytes, kept counts, slot offsets,
row-index entries, thresholds, bounds and histogram bins: bit for bit.  Cells and
flat arrays: test_gpu_fuzz.same_cells (bit for bit, a NaN matching any NaN).
RMSE: max(1e-12, (n + 4) 2^-53) relative, NaN where the oracle's is, the bound
tests/test_gpu_fuzz.py derives.  Every output buffer is prefilled: payload
buffers with zeros and compared WHOLE (slots, the bytes between them and the
bytes past the last one), cell-shaped buffers and the row index with a
sentinel that must survive wherever the call promises not to write (the gaps
between units; the row entries of units that are not of the row-indexed shape).
No unit is left out of any comparison.

Fields: (a) the smooth SURVEY field on every unit; (b) test_gpu_fuzz._field with
kind = i % 8 (long_axis_shapes.fuzz_box).  The oracle's results are computed once
per (field, keep) and shared."""
import numpy as np
import pytest

import long_axis_shapes as S
import modes_batches as M
import numpy_ref
from test_gpu_coarse import Case
from test_gpu_coarse import Dev as CoarseDev
from test_gpu_fuzz import same_cells
from test_gpu_modes_fuzz import LevelsCase, TolCase, check_tol, options, rmse_agrees, run_levels_device, run_levels_host
from test_gpu_rix_options import SENTINEL
from test_gpu_tol import Dev as TolDev
from tol_rule import MARGIN, field
from wavelet_compression_amd.capi import WC_OPT_HOST_CHUNK, WC_OPT_TOL_SOLO_TILES

pytestmark = pytest.mark.gpu

KEEP = float(np.float32(0.999))
ROW_SENTINEL = 0xA5A5A5A5
CASES = [("a", np.float64, KEEP), ("a", np.float64, 1.0), ("a", np.float32, KEEP), ("a", np.float32, 1.0),
         ("b", np.float64, KEEP), ("b", np.float32, KEEP)]
_ids = [f"{w}-{np.dtype(t).name}-keep{k:g}" for w, t, k in CASES]

_boxes, _oracle_results = {}, {}


class Ref:
    """One batch (a list of long_axis_shapes units, a field, a cell type, a keep) with
    the oracle's results: payloads, reconstructions and RMSEs, computed once per
    (units, field, keep) and left unchanged."""

    def __init__(self, wc, O, which, dtype, keep, extra=()):
        self.spec = S.UNITS + list(extra)
        self.tags, self.dims = [t for t, _ in self.spec], [d for _, d in self.spec]
        self.offs, self.extent = S.layout(self.spec)
        self.units, self.n, ext = wc.capi.make_units(self.dims, offsets=self.offs)
        assert ext == self.extent
        self.dtype, self.keep, self.which = dtype, keep, which
        self.code = wc.capi.WC_F64 if dtype == np.float64 else wc.capi.WC_F32
        self.total = (self.extent + 8 + 3) & ~3  # sentinels behind the last unit too; stacked outputs stay 16-B aligned
        key = (which, len(self.spec))
        if key not in _boxes:
            _boxes[key] = S.boxes(O, self.spec, which)
        self.boxes = _boxes[key]
        self.b32 = [M.narrow(O, b, dtype) for b in self.boxes]
        self.sizes = [b.size for b in self.boxes]
        self.inside = np.zeros(self.total, bool)
        for o, sz in zip(self.offs, self.sizes):
            self.inside[o:o + sz] = True
        # the oracle: shared between the cell types when both narrow to the same fp32 cells
        okey = (which, len(self.spec), keep)
        have = _oracle_results.get(okey)
        if have is None or any(a.tobytes() != b.tobytes() for a, b in zip(have["b32"], self.b32)):
            have = self._run_oracle(O)
            _oracle_results.setdefault(okey, have)
        self.payloads, self.kept, self.back, self.ref_rmse = have["payloads"], have["kept"], have["back"], have["rmse"]
        self.want = np.full(self.total, SENTINEL, np.uint32).view(np.float32)
        for o, bk in zip(self.offs, self.back):
            self.want[o:o + bk.size] = bk.ravel()

    def _run_oracle(self, O):
        payloads, kept, back, rmse = [], [], [], []
        with np.errstate(all="ignore"):
            for b in self.b32:
                p, k = O.compress_payload(b, self.keep)
                payloads.append(p)
                kept.append(k)
                bk = O.decompress_payload(p) if b.size else b
                back.append(bk)
                rmse.append(O.rmse(b, bk) if b.size else 0.0)
        return dict(b32=self.b32, payloads=payloads, kept=kept, back=back, rmse=rmse)

    def host_cells(self):
        h = np.zeros(self.total, self.dtype)
        for o, b in zip(self.offs, self.boxes):
            h[o:o + b.size] = b.ravel().astype(self.dtype)
        return h

    def slots(self, idx=None):
        """Slot offsets of wc_forward for the units idx (default: all), and the end of the last slot."""
        pos, out = 4, []
        for i in (range(self.n) if idx is None else idx):
            out.append(pos)
            pos += 24 + 8 * self.sizes[i]
        return out, pos

    def want_payload(self, cap, idx=None):
        """The whole payload buffer of wc_forward over zeros: every slot, nothing between them."""
        idx = list(range(self.n)) if idx is None else idx
        buf = np.zeros(cap, np.uint8)
        slots, end = self.slots(idx)
        assert end <= cap
        for s, i in zip(slots, idx):
            buf[s:s + len(self.payloads[i])] = np.frombuffer(self.payloads[i], np.uint8)
        offsets = np.array(slots + [slots[-1] + 20 + 8 * self.kept[idx[-1]]], np.uint64)
        return buf, offsets, np.array([self.kept[i] for i in idx], np.uint32)

    def want_rows(self, entries):
        """The whole row index of wc_forward_rows over the sentinel: the entries of every unit
        of the row-indexed shape as the header defines them ({k, p_k - r D}, closing {nrle,
        ncoeff - r D}; numpy_ref.row_index), the other units' entries not written."""
        rows = np.full((entries, 2), ROW_SENTINEL, np.uint32)
        ent = 0
        for (W, H, D), p, sz in zip(self.dims, self.payloads, self.sizes):
            if sz and W % 2 == 0 and H % 2 == 0 and D % 8 == 0:
                rows[ent:ent + W * H + 1] = numpy_ref.row_index(p, W, H, D)
            if sz:
                ent += W * H + 1
        assert ent == entries
        return rows

    def want_cells(self, idx):
        w = np.full(self.total, SENTINEL, np.uint32).view(np.float32)
        for i in idx:
            o = self.offs[i]
            w[o:o + self.sizes[i]] = self.back[i].ravel()
        return w

    def where(self, got, want):
        """The units whose cells differ, and the overwritten cells outside the units."""
        bad = [f"unit {i} {self.tags[i]} {self.dims[i]}" for i, (o, sz) in enumerate(zip(self.offs, self.sizes))
               if sz and not same_cells(got[o:o + sz], want[o:o + sz])]
        hit = np.flatnonzero(~self.inside & (got.view(np.uint32) != want.view(np.uint32)))
        if hit.size:
            bad.append(f"{hit.size} cells outside the units overwritten, first at element {hit[0]}")
        return bad


_refs = {}


def ref_for(wc, O, which, dtype, keep, extra=()):
    key = (which, np.dtype(dtype).name, keep, len(extra))
    if key not in _refs:
        _refs[key] = Ref(wc, O, which, dtype, keep, extra)
    return _refs[key]


def sentinel_cells(shape):
    import torch
    return torch.full(shape, SENTINEL - (1 << 32), dtype=torch.int32, device=torch.device("cuda", 0)).view(torch.float32)


def check_rmse(ref, E, idx, what):
    return [f"{what}: unit {i} {ref.tags[i]} {ref.dims[i]} rmse {E[j]!r}, oracle {ref.ref_rmse[i]!r}"
            for j, i in enumerate(idx) if not rmse_agrees(E[j], ref.ref_rmse[i], ref.sizes[i])]


def profiled(ctx, call):
    """The stages a call launched (wc_profile_read)."""
    ctx.synchronize()
    ctx.profile_enable(True)
    try:
        ctx.profile_read()
        call()
        ctx.synchronize()
        return set(ctx.profile_read())
    finally:
        ctx.profile_enable(False)


def run_payload_paths(wc, ctx, ref, what, fused_at=None):
    """wc_forward, wc_forward_rows, wc_inverse, wc_inverse_rows (the forward's row index, then
    NULL), wc_inverse_rmse on the whole (mixed) batch; with fused_at (a WC_OPT_RIX_LDS budget)
    also wc_forward + wc_inverse_rmse on the sub-batch of the units that are row-indexed at that
    budget, where the RMSE is fused into the row-indexed inverse.  -> (failures, results)."""
    import torch
    dev = torch.device("cuda", 0)
    units, n = ref.units, ref.n
    cells = torch.from_numpy(ref.host_cells()).to(dev)
    cap = wc.capi.payload_bound(units, n)
    rb = wc.capi.rowindex_bytes(units, n)

    def bufs(m, c):
        return (torch.zeros(c, dtype=torch.uint8, device=dev), torch.full((m + 1,), -3, dtype=torch.int64, device=dev),
                torch.full((m,), -1, dtype=torch.int32, device=dev))

    pay, po, kept = bufs(n, cap)
    pay2, po2, kept2 = bufs(n, cap)
    rows = torch.full((rb // 4,), ROW_SENTINEL - (1 << 32), dtype=torch.int32, device=dev)
    out = sentinel_cells((5, ref.total))
    rmse = torch.full((2, n), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()  # the fills run on torch's stream, the context on its own
    ctx.forward(cells.data_ptr(), ref.code, units, n, ref.keep, pay.data_ptr(), cap, po.data_ptr(), kept.data_ptr())
    ctx.forward_rows(cells.data_ptr(), ref.code, units, n, ref.keep, pay2.data_ptr(), cap, po2.data_ptr(),
                     kept2.data_ptr(), rows.data_ptr(), rb)
    ctx.inverse(pay.data_ptr(), po.data_ptr(), units, n, out[0].data_ptr())
    ctx.inverse_rows(pay2.data_ptr(), po2.data_ptr(), units, n, rows.data_ptr(), out[1].data_ptr(), rowinfo_capacity=rb)
    ctx.inverse_rows(pay2.data_ptr(), po2.data_ptr(), units, n, None, out[2].data_ptr())
    stages = profiled(ctx, lambda: ctx.inverse_rmse(pay.data_ptr(), po.data_ptr(), units, n, cells.data_ptr(), ref.code,
                                                    out[3].data_ptr(), rmse[0].data_ptr()))
    bad = []
    if "rmse" not in stages:  # a batch with dense-decode units: wc_inverse + wc_rmse
        bad.append(f"{what}: wc_inverse_rmse on the mixed batch ran the stages {sorted(stages)}")
    sub = None
    if fused_at is not None:
        sub = [i for i, t in enumerate(ref.tags) if S.CLASSES[t][f"rix{fused_at}"] or not ref.sizes[i]]
        assert 0 < len(sub) < n and any(not ref.sizes[i] for i in sub)
        su, sn, _ = wc.capi.make_units([ref.dims[i] for i in sub], offsets=[ref.offs[i] for i in sub])
        scap = wc.capi.payload_bound(su, sn)
        spay, spo, skept = bufs(sn, scap)
        torch.cuda.synchronize()
        ctx.forward(cells.data_ptr(), ref.code, su, sn, ref.keep, spay.data_ptr(), scap, spo.data_ptr(), skept.data_ptr())
        stages = profiled(ctx, lambda: ctx.inverse_rmse(spay.data_ptr(), spo.data_ptr(), su, sn, cells.data_ptr(), ref.code,
                                                        out[4].data_ptr(), rmse[1].data_ptr()))
        if "rmse" in stages or "inverse" not in stages:  # every unit row-indexed: the RMSE is fused
            bad.append(f"{what}: wc_inverse_rmse on the all-fast sub-batch ran the stages {sorted(stages)}")
    ctx.synchronize()

    want_pay, want_off, want_kept = ref.want_payload(cap)
    P = pay.cpu().numpy()
    res = dict(P=P, cells=out[0].cpu().numpy())
    for tag, p, o, k in (("wc_forward", P, po, kept), ("wc_forward_rows", pay2.cpu().numpy(), po2, kept2)):
        O_, K = o.cpu().numpy().view(np.uint64), k.cpu().numpy().view(np.uint32)
        if not np.array_equal(O_, want_off):
            bad.append(f"{what}: {tag}: slot offsets differ, first at unit {int(np.flatnonzero(O_ != want_off)[0])}")
        if not np.array_equal(K, want_kept):
            i = int(np.flatnonzero(K != want_kept)[0])
            bad.append(f"{what}: {tag}: kept counts differ, first at unit {i} {ref.tags[i]}: {K[i]}, oracle {want_kept[i]}")
        if not np.array_equal(p, want_pay):
            slots, end = ref.slots()
            at = int(np.flatnonzero(p != want_pay)[0])
            i = int(np.searchsorted(np.array(slots), at, side="right")) - 1
            bad.append(f"{what}: {tag}: payload bytes differ from the oracle's, first at byte {at}: unit {i} "
                       f"{ref.tags[max(i, 0)]} {ref.dims[max(i, 0)]}, byte {at - slots[max(i, 0)]} of its slot")
    got_rows = rows.cpu().numpy().view(np.uint32).reshape(-1, 2)
    want_rows = ref.want_rows(rb // 8)
    if not np.array_equal(got_rows, want_rows):
        ent = 0
        for i, ((W, H, D), sz) in enumerate(zip(ref.dims, ref.sizes)):
            cnt = W * H + 1 if sz else 0
            if not np.array_equal(got_rows[ent:ent + cnt], want_rows[ent:ent + cnt]):
                r = int(np.flatnonzero((got_rows[ent:ent + cnt] != want_rows[ent:ent + cnt]).any(axis=1))[0])
                bad.append(f"{what}: wc_forward_rows: row index of unit {i} {ref.tags[i]} {ref.dims[i]} differs, first at "
                           f"row {r}: {got_rows[ent + r].tolist()}, expected {want_rows[ent + r].tolist()}")
            ent += cnt
    got = out.cpu().numpy()
    for c, call in enumerate(("wc_inverse", "wc_inverse_rows", "wc_inverse_rows NULL", "wc_inverse_rmse mixed")):
        if not same_cells(got[c], ref.want):
            bad += [f"{what}: {call}: {b}" for b in ref.where(got[c], ref.want)]
    E = rmse.cpu().numpy()
    bad += check_rmse(ref, E[0], range(n), f"{what}: wc_inverse_rmse mixed")
    if sub is not None:
        want_sub = ref.want_cells(sub)
        if not same_cells(got[4], want_sub):
            bad += [f"{what}: wc_inverse_rmse fused: {b}" for b in ref.where(got[4], want_sub)]
        bad += check_rmse(ref, E[1][:len(sub)], sub, f"{what}: wc_inverse_rmse fused")
        sp, so, sk = ref.want_payload(scap, sub)
        if not (np.array_equal(spay.cpu().numpy(), sp) and np.array_equal(spo.cpu().numpy().view(np.uint64), so)
                and np.array_equal(skept.cpu().numpy().view(np.uint32), sk)):
            bad.append(f"{what}: wc_forward on the all-fast sub-batch differs from the oracle")
    return bad, res


@pytest.mark.parametrize("which,dtype,keep", CASES, ids=_ids)
def test_forward_and_inverses(wc, ctx, oracle, which, dtype, keep):
    ref = ref_for(wc, oracle, which, dtype, keep)
    bad, _ = run_payload_paths(wc, ctx, ref, f"field ({which}) {np.dtype(dtype).name} keep {keep:g}", fused_at=9216)
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("which,dtype", [(w, t) for w, t, k in CASES if k == KEEP], ids=[i for i, c in zip(_ids, CASES) if c[2] == KEEP])
def test_transforms_and_rmse(wc, ctx, oracle, which, dtype):
    """wc_decompose and wc_inverse_flat (the oracle's flat arrays through the synthesis alone)
    on the same units; wc_rmse of the oracle's reconstruction with the original cells at an odd
    element offset (8 bytes past a 16-B boundary for fp64, 4 for fp32)."""
    import torch
    ref = ref_for(wc, oracle, which, dtype, KEEP)
    dev = torch.device("cuda", 0)
    units, n = ref.units, ref.n
    host = ref.host_cells()
    shifted = torch.zeros(ref.total + 1, dtype=torch.float64 if dtype == np.float64 else torch.float32, device=dev)
    shifted[1:] = torch.from_numpy(host).to(dev)
    cells = shifted[1:]
    assert cells.data_ptr() % 16 == shifted.element_size()
    aligned = torch.from_numpy(host).to(dev)
    flat_want = np.full(ref.total, SENTINEL, np.uint32).view(np.float32)
    synth_want = flat_want.copy()
    with np.errstate(all="ignore"):
        for (W, H, D), o, b in zip(ref.dims, ref.offs, ref.b32):
            if b.size:
                f = oracle.wavelet_decompose(b)
                flat_want[o:o + b.size] = f
                synth_want[o:o + b.size] = oracle.inverse_wavelet_decompose(f, W, H, D).ravel()
    out = sentinel_cells((2, ref.total))
    flat_in = torch.from_numpy(flat_want).to(dev)
    regen = torch.from_numpy(ref.want).to(dev)
    rmse = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.decompose(aligned.data_ptr(), ref.code, units, n, out[0].data_ptr())
    ctx.inverse_flat(flat_in.data_ptr(), units, n, out[1].data_ptr())
    ctx.rmse(cells.data_ptr(), ref.code, regen.data_ptr(), units, n, rmse.data_ptr())
    ctx.synchronize()
    got = out.cpu().numpy()
    bad = []
    for c, (call, want) in enumerate((("wc_decompose", flat_want), ("wc_inverse_flat", synth_want))):
        if not same_cells(got[c], want):
            bad += [f"{call}: {b}" for b in ref.where(got[c], want)]
    bad += check_rmse(ref, rmse.cpu().numpy(), range(n), "wc_rmse, odd offset")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:40])


# Field (a), keep 0.999, fp32: payloads and cells identical to the default leg's and the oracle's.
OPTION_LEGS = {
    "dense_staging": (("WC_OPT_SPARSE", 0),),
    "tickets": (("WC_OPT_TICKETS", 1),),
    "reversed_spin_1": (("WC_OPT_REVERSE_TILES", 1), ("WC_OPT_SPIN_LIMIT", 1)),
    "dense_inverse": (("WC_OPT_INVERSE_ROWS", 0),),
    "rix_lds_16384": (("WC_OPT_RIX_LDS", 16384),),  # with the two units of the 16384 boundary appended
    "rix_lds_1024": (("WC_OPT_RIX_LDS", 1024),),    # every D > 232 decodes densely
    "inv_groups_3": (("WC_OPT_INV_GROUPS", 3),),
    "rix_xcd": (("WC_OPT_RIX_XCD", 1),),
}
_default_leg = {}


def default_leg(wc, ctx, oracle):
    if not _default_leg:
        ref = ref_for(wc, oracle, "a", np.float32, KEEP)
        bad, res = run_payload_paths(wc, ctx, ref, "default leg")
        assert not bad, "\n".join(bad[:40])
        _default_leg.update(res, end=ref.slots()[1], extent=ref.extent)
    return _default_leg


@pytest.mark.parametrize("leg", sorted(OPTION_LEGS))
def test_option_legs(wc, ctx, oracle, leg):
    base = default_leg(wc, ctx, oracle)
    extra = S.RIX16K if leg == "rix_lds_16384" else ()
    ref = ref_for(wc, oracle, "a", np.float32, KEEP, extra)
    with options(wc, ctx, OPTION_LEGS[leg]):
        bad, res = run_payload_paths(wc, ctx, ref, leg, fused_at=16384 if leg == "rix_lds_16384" else None)
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:40])
    # the default leg's bytes (the appended units lie behind the default batch in both buffers)
    assert np.array_equal(res["P"][:base["end"]], base["P"][:base["end"]]), leg
    assert res["cells"][:base["extent"]].tobytes() == base["cells"][:base["extent"]].tobytes(), leg


@pytest.mark.parametrize("which,dtype", [("a", np.float64), ("b", np.float32)], ids=["a-float64", "b-float32"])
def test_host_forms(wc, ctx, oracle, which, dtype):
    """wc_forward_host, wc_inverse_host and wc_round_trip_host with WC_OPT_HOST_CHUNK = 2^18: the
    batch splits into unit runs between the long units.  Packed payloads, the oracle's bytes,
    cells and RMSEs; cells no unit owns keep what the caller's buffer held."""
    ref = ref_for(wc, oracle, which, dtype, KEEP)
    host = ref.host_cells()
    out = np.full(ref.total, SENTINEL, np.uint32).view(np.float32)
    with options(wc, ctx, [(WC_OPT_HOST_CHUNK, 1 << 18)]):
        pay, po, kept = ctx.forward_host(host, ref.units, ref.n, KEEP)
        pay_r, po_r, kept_r, rmse = ctx.round_trip_host(host, ref.units, ref.n, KEEP)
        regen = ctx.inverse_host(pay, po[:ref.n], ref.units, ref.n, ref.total, out=out)
    bad = []
    for tag, (p, o, k) in (("wc_forward_host", (pay, po, kept)), ("wc_round_trip_host", (pay_r, po_r, kept_r))):
        pos = 4
        for i in range(ref.n):
            if int(o[i]) != pos or int(k[i]) != ref.kept[i] or wc.capi.unit_payload(p, o, k, i) != ref.payloads[i]:
                bad.append(f"{tag}: unit {i} {ref.tags[i]} {ref.dims[i]}: offset {int(o[i])} (packed: {pos}), kept {int(k[i])} "
                           f"(oracle: {ref.kept[i]}), payload equal: {wc.capi.unit_payload(p, o, k, i) == ref.payloads[i]}")
            pos += 24 + 8 * ref.kept[i]
        if int(o[ref.n]) != pos - 4:
            bad.append(f"{tag}: offsets[n] {int(o[ref.n])}, the last unit's bytes end at {pos - 4}")
    if not same_cells(regen, ref.want):
        bad += [f"wc_inverse_host: {b}" for b in ref.where(regen, ref.want)]
    bad += check_rmse(ref, rmse, range(ref.n), "wc_round_trip_host")
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:40])


# ---- the opt-in modes ---------------------------------------------------------------------------

_levels = {}


def levels_case(wc, oracle, which):
    """The levels list as a test_gpu_modes_fuzz.LevelsCase: field (a) as fp64 cells, field (b)
    as fp32 cells with the kinds (i + 3) % 8 (a Gaussian, a constant, zeros, subnormals, the
    NaN / inf sprinkles, the smooth field)."""
    if which not in _levels:
        spec = [(f"levels{i}", d) for i, (d, _) in enumerate(S.LEVELS)]
        LB = M.LevelsBatch()
        LB.seed, LB.dtype = 0, (np.float64 if which == "a" else np.float32)
        LB.dims, LB.levels = [d for d, _ in S.LEVELS], [L for _, L in S.LEVELS]
        LB.offsets, LB.extent = S.layout(spec)
        if which == "a":
            LB.boxes = [S.survey_box(oracle, 100 + i, d) for i, d in enumerate(LB.dims)]
        else:
            LB.boxes = [S.fuzz_box(oracle, i, d, kind=(i + 3) % 8) for i, d in enumerate(LB.dims)]
        LB.n, LB.keep, LB.tags = len(spec), KEEP, {}
        _levels[which] = LevelsCase(wc, oracle, LB)
    return _levels[which]


@pytest.mark.parametrize("which", ["a", "b"])
def test_levels(wc, ctx, oracle, which):
    """wc_decompose_levels, wc_inverse_flat_levels, wc_forward_levels at keep 0.999 and with an
    explicit threshold, wc_inverse_levels and the _host forms on the levels list, against
    levels_ref: level passes on sub-boxes such as 1024 x 8 x 8 (two work items of 4096 blocks)."""
    B = levels_case(wc, oracle, which)
    run_levels_device(wc, ctx, B, ("long axis", which))
    run_levels_host(wc, ctx, B, 1 << 18)


COARSE_L1 = ["magic_d_y", "rix_edge_in", "magic_d_3000", "big_x"]  # 2 x 130 x 1000, 2 x 2 x 2280, 8 x 8 x 3000, 2048 x 32 x 32


def coarse_payloads(wc, oracle):
    """The levels list's payloads (field (a), keep 0.999) at every r in 0..L, then the one-level
    payloads of COARSE_L1 at r = 1."""
    B = levels_case(wc, oracle, "a")
    ref = ref_for(wc, oracle, "a", np.float64, KEEP)
    pays, reduce = [], []
    for i, L in enumerate(B.levels):
        for r in range(L + 1):
            pays.append(B.payload(i, KEEP)[0])
            reduce.append(r)
    for t in COARSE_L1:
        pays.append(ref.payloads[ref.tags.index(t)])
        reduce.append(1)
    return pays, reduce


def run_coarse(ctx, case, d):
    ctx.inverse_coarse(d.pay.data_ptr(), d.off.data_ptr(), case.units, case.n, case.levels, case.reduce, case.out_units,
                       d.out.data_ptr())


def test_coarse(wc, ctx, oracle):
    """wc_inverse_coarse against coarse_ref.  The corner filter divides flat positions by D
    and rows by H in the multiply form: D = 1000, 2280, 3000, 4000 and H = 130 are no powers of
    two."""
    pays, reduce = coarse_payloads(wc, oracle)
    case = Case(wc, pays, reduce, odd_at=7)
    assert case.out_units[7].cell_offset % 2 == 1
    d = CoarseDev(case)
    run_coarse(ctx, case, d)
    ctx.synchronize()
    case.check(d.out.cpu().numpy(), what="long axis")


def test_coarse_negative_run_in_the_second_pair_tile(wc, ctx, oracle):
    """A negative run planted in the second pair tile (pairs 4096..8191) of 2 x 130 x 1000:
    WC_ERR_FORMAT (the negative-run bit alone) at the next wc_synchronize, the other units
    decoded, nothing written outside the unit's own range."""
    pays, reduce = coarse_payloads(wc, oracle)
    good = Case(wc, pays, reduce)
    i = len(pays) - len(COARSE_L1) + COARSE_L1.index("magic_d_y")
    (W, H, D), nc, runs, vals = oracle.parse_payload(pays[i])
    assert (W, H, D) == (2, 130, 1000) and len(runs) > 2 * 4096
    runs = runs.copy()
    runs[4096 + 100] = -2
    case = Case.__new__(Case)
    case.__dict__.update(good.__dict__)
    case.buf = good.buf.copy()
    o = int(good.offsets[i])
    case.buf[o:o + len(pays[i])] = np.frombuffer(oracle.serialize(W, H, D, nc, runs, vals), np.uint8)
    d = CoarseDev(case)
    run_coarse(ctx, case, d)
    with pytest.raises(wc.WaveletError) as ei:
        ctx.synchronize()
    assert ei.value.code == wc.capi.WC_ERR_FORMAT and "flags 0x2" in str(ei.value)
    ctx.synchronize()  # the error word is cleared
    case.check(d.out.cpu().numpy(), what="negative run", skip=(i,))
    d2 = CoarseDev(good)  # the context goes on
    run_coarse(ctx, good, d2)
    ctx.synchronize()
    good.check(d2.out.cpu().numpy(), what="after the negative run")


TOLS = (0.0, 1e-3, 0.1, np.inf)
_tol = {}


def tol_case(wc, oracle):
    """The even-dims units of the list (each once, with cells) with tol_rule.field's cells
    (|x| <= 8: the fields MARGIN is derived for), fp32."""
    if not _tol:
        spec = [(t, d) for t, d in S.UNITS if S.CLASSES[t]["fast"] and not t.endswith("_odd")]
        assert all(not (d[0] | d[1] | d[2]) & 1 for _, d in spec)
        assert len(spec) == sum(1 for t, d in S.UNITS if d[0] * d[1] * d[2] and not (d[0] | d[1] | d[2]) & 1) - len(S.S32_TAGS)
        TB = M.TolBatch()
        TB.seed, TB.dtype = 0, np.float32
        TB.dims, TB.n = [d for _, d in spec], len(spec)
        TB.boxes = [field(i % 3, *d, seed=200 + i) for i, d in enumerate(TB.dims)]
        TB.offsets, TB.extent = S.layout(spec)
        TB.tol = [TOLS[i % 4] for i in range(TB.n)]
        _tol["case"] = TolCase(wc, oracle, TB)
    return _tol["case"]


@pytest.mark.parametrize("solo_tiles", [64, 1])
def test_tol(wc, ctx, oracle, solo_tiles):
    """wc_forward_tol, then wc_forward_stage + wc_forward_emit_tol three times with the
    tolerances rotated, so that every unit meets 0, 1e-3, 0.1 and inf; binned by one workgroup
    per unit of at most 64 flat tiles (the longer units split) and with every unit of more than
    one tile split.  Thresholds and bounds bit for bit, the payloads of tol_rule's threshold; the
    actual RMSE of each round trip (wc_inverse_rmse) within tol (1 + MARGIN) for tol >= 1e-3."""
    import torch
    T = tol_case(wc, oracle)
    assert any(w * h * d > 64 * 4096 for w, h, d in T.dims) and any(4096 < w * h * d <= 64 * 4096 for w, h, d in T.dims)
    dev = torch.device("cuda", 0)
    out = torch.zeros(max(T.extent, 1), dtype=torch.float32, device=dev)
    rmse = torch.zeros(T.n, dtype=torch.float64, device=dev)
    with options(wc, ctx, [(WC_OPT_TOL_SOLO_TILES, solo_tiles)]):
        for k in range(4):
            tols = [TOLS[(i + k) % 4] for i in range(T.n)]
            d = TolDev(wc, T.cells, T.units, T.n)
            if k == 0:
                ctx.forward_tol(d.cells.data_ptr(), d.dtype, T.units, T.n, tols, *d.out_args())
            else:
                ctx.forward_stage(d.cells.data_ptr(), d.dtype, T.units, T.n, None)
                ctx.forward_emit_tol(T.units, T.n, tols, *d.out_args())
            ctx.synchronize()
            check_tol(T, d.read(), tols, ("long axis", solo_tiles, k))
            ctx.inverse_rmse(d.pay.data_ptr(), d.off.data_ptr(), T.units, T.n, d.cells.data_ptr(), d.dtype, out.data_ptr(),
                             rmse.data_ptr())
            ctx.synchronize()
            E = rmse.cpu().numpy()
            for i, t in enumerate(tols):
                if 1e-3 <= t < np.inf:
                    assert E[i] <= t * (1 + MARGIN), (solo_tiles, k, i, T.dims[i], t, E[i])


@pytest.mark.parametrize("which,dtype", [("a", np.float32), ("b", np.float64)], ids=["a-float32", "b-float64"])
def test_histogram_threshold_emit(wc, ctx, oracle, which, dtype):
    """wc_forward_stage with a histogram, wc_hist_threshold at quantile 0.9, wc_forward_emit with
    that threshold: the bins equal the summed oracle.magnitude_hist, the payloads equal
    compress_payload_thresh."""
    import torch
    ref = ref_for(wc, oracle, which, dtype, KEEP)
    dev = torch.device("cuda", 0)
    units, n = ref.units, ref.n
    cells = torch.from_numpy(ref.host_cells()).to(dev)
    cap = wc.capi.payload_bound(units, n)
    hist = torch.zeros(wc.capi.HIST_BINS, dtype=torch.int64, device=dev)
    pay = torch.zeros(cap, dtype=torch.uint8, device=dev)
    po = torch.full((n + 1,), -3, dtype=torch.int64, device=dev)
    kept = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.forward_stage(cells.data_ptr(), ref.code, units, n, hist.data_ptr())
    ctx.synchronize()
    h = hist.cpu().numpy().view(np.uint64)
    with np.errstate(all="ignore"):
        want = sum(oracle.magnitude_hist(oracle.wavelet_decompose(b)) for b in ref.b32 if b.size)
    assert np.array_equal(h, want.astype(np.uint64)), np.flatnonzero(h != want)[:8]
    t, r = wc.capi.hist_threshold(h, 0.9)
    ctx.forward_emit(units, n, 0.0, t, pay.data_ptr(), cap, po.data_ptr(), kept.data_ptr())
    ctx.synchronize()
    P, O_, K = pay.cpu().numpy(), po.cpu().numpy().view(np.uint64), kept.cpu().numpy().view(np.uint32)
    assert int(K.astype(np.int64).sum()) == r
    want_pay = np.zeros(cap, np.uint8)
    slots, _ = ref.slots()
    with np.errstate(all="ignore"):
        for i, (b, s, (W, H, D)) in enumerate(zip(ref.b32, slots, ref.dims)):
            p = oracle.compress_payload_thresh(b, t) if b.size else oracle.serialize(W, H, D, 0, [], [])
            assert int(O_[i]) == s and int(K[i]) == (len(p) - 20) // 8, (i, ref.tags[i])
            want_pay[s:s + len(p)] = np.frombuffer(p, np.uint8)
    if not np.array_equal(P, want_pay):
        at = int(np.flatnonzero(P != want_pay)[0])
        i = int(np.searchsorted(np.array(slots), at, side="right")) - 1
        raise AssertionError(f"payload bytes differ first at byte {at}: unit {i} {ref.tags[max(i, 0)]} {ref.dims[max(i, 0)]}")
