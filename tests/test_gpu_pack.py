"""GPU: the packed payload transcoders (include/wavelet_amd.h wc_pack, wc_unpack,
wc_pack_host, wc_unpack_host; codec pack=) against the numpy restatement
tests/pack_rule.py.

Bar: byte for byte.  Packed bytes, exact lengths and offsets equal the
restatement's; every byte of a sentinel-prefilled buffer outside a unit's exact
length keeps its sentinel; wc_unpack(wc_pack(p)) is p at V = 4 and the
restatement's quantised payload at V = 2, 3; the decoders on unpacked payloads
give the references' cells on the quantised payload.

One batch (pack_rule.batch): field units of 8^3 up to 32x16x8 cells at L = 1..3
with 0, 1, 63, 64, 65, 128 pairs and 2047, 2048, 2049 (the tile is 2048 pairs),
a unit without cells, a fully kept noise unit (every width 0), a constant box,
three payloads made by hand on an 8^3 unit (w = 31, a chunk of mixed widths, the
special values) and one 64^3 unit at keep 0.999 (several tiles of one unit)."""
import functools

import numpy as np
import pytest

import coarse_ref as CR
import levels_ref as LR
import pack_rule as PR
import region_ref as RR

pytestmark = pytest.mark.gpu

SENT = 0xA5
VS = (2, 3, 4)


class Batch:
    """Payloads in the forward's slot layout, with the restatement's packed units
    and quantised payloads per V (computed once, left unchanged)."""

    def __init__(self, wc, units, vs=VS, restated=None):
        self.what = [u[0] for u in units]
        self.pays = [u[1] for u in units]
        self.n = len(self.pays)
        self.dims = [tuple(int(v) for v in np.frombuffer(p[:12], np.int32)) for p in self.pays]
        self.levels = [PR.parse(p)[3] for p in self.pays]
        self.units, _, self.extent = wc.capi.make_units(self.dims)
        self.pay_off, self.pay_cap = PR.payload_slots(self.dims)
        self.buf = self.layout(self.pays, self.pay_off, self.pay_cap)
        packed, quant = restated or ({V: [PR.pack(p, V) for p in self.pays] for V in vs},
                                     {V: [PR.quantise(p, V) for p in self.pays] for V in vs})
        self.packed, self.quant = packed, quant
        self.slots = {V: PR.slot_offsets(self.dims, V) for V in vs}

    def head(self, wc, k):
        """The first k units as a batch of their own; the restatement's bytes are shared, not computed again."""
        units = list(zip(self.what[:k], self.pays[:k]))
        return Batch(wc, units, vs=tuple(self.packed), restated=({V: p[:k] for V, p in self.packed.items()},
                                                                 {V: q[:k] for V, q in self.quant.items()}))

    @staticmethod
    def layout(items, offs, cap, margin=64):
        buf = np.full(cap + margin, SENT, np.uint8)
        for p, o in zip(items, offs):
            buf[o:o + len(p)] = np.frombuffer(p, np.uint8)
        return buf

    def dense(self, V):
        """The packed units back to back (each at 4 mod 8), as wc_pack_host lays them out."""
        off = [4]
        for p in self.packed[V]:
            off.append(off[-1] + PR.pad8(len(p)))
        end = off[-2] + len(self.packed[V][-1])
        return self.layout(self.packed[V], off[:-1], end, margin=0), off[:-1], end


@pytest.fixture(scope="module", params=["f32", "f64"])
def B(request, wc):
    return Batch(wc, PR.batch(request.param))


@pytest.fixture(scope="module")
def BN(wc):
    """The field units alone (finite values, runs inside the box): what the decoders are run on."""
    return Batch(wc, [u for u in PR.batch("f32") if u[2]])


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def filled(nbytes):
    import torch
    t = torch.full((nbytes,), SENT, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def u64(a):
    return dev(np.asarray(a, np.uint64))


def host(t, dtype=np.uint8):
    return t.cpu().numpy().view(dtype)


def run_pack(ctx, B, V, d_pay=None, d_off=None, sync=True):
    cap = B.slots[V][1]
    out = filled(cap + 64)
    poff, pbytes = filled(8 * (B.n + 1)), filled(8 * B.n)
    d_pay = dev(B.buf) if d_pay is None else d_pay
    d_off = u64(B.pay_off) if d_off is None else d_off
    ctx.pack(d_pay.data_ptr(), d_off.data_ptr(), B.units, B.n, V, out.data_ptr(), cap, poff.data_ptr(), pbytes.data_ptr())
    if sync:
        ctx.synchronize()
    return out, poff, pbytes, (d_pay, d_off)


def run_unpack(ctx, B, d_packed, d_poff, pcap, sync=True):
    out = filled(B.pay_cap + 64)
    off, kept = filled(8 * (B.n + 1)), filled(4 * B.n)
    ctx.unpack(d_packed.data_ptr(), d_poff.data_ptr(), pcap, B.units, B.n, out.data_ptr(), B.pay_cap, off.data_ptr(),
               kept.data_ptr())
    if sync:
        ctx.synchronize()
    return out, off, kept


def check_packed(B, V, out, poff, pbytes, skip=()):
    got, off, nb = host(out), host(poff, np.uint64), host(pbytes, np.uint64)
    slots, cap = B.slots[V]
    assert off[:B.n].tolist() == slots
    owned = np.zeros(got.size, bool)
    for i, want in enumerate(B.packed[V]):
        if i in skip:
            owned[slots[i]:slots[i] + PR.pad8(PR.worst(np.prod(B.dims[i], dtype=np.int64), V) + 4) - 4] = True
            continue
        assert int(nb[i]) == len(want), (B.what[i], V)
        assert got[slots[i]:slots[i] + len(want)].tobytes() == want, (B.what[i], V)
        owned[slots[i]:slots[i] + len(want)] = True
    if B.n - 1 not in skip:
        assert int(off[B.n]) == slots[-1] + len(B.packed[V][-1])
    assert np.all(got[~owned] == SENT), V  # nothing outside each unit's exact length


def check_unpacked(B, want, out, off, kept, skip=()):
    got, o, k = host(out), host(off, np.uint64), host(kept, np.uint32)
    assert o[:B.n].tolist() == B.pay_off
    owned = np.zeros(got.size, bool)
    for i, w in enumerate(want):
        if i in skip:
            owned[B.pay_off[i]:B.pay_off[i] + 20 + 8 * int(np.prod(B.dims[i], dtype=np.int64))] = True
            continue
        assert int(k[i]) == (len(w) - 20) // 8, B.what[i]
        assert got[B.pay_off[i]:B.pay_off[i] + len(w)].tobytes() == w, B.what[i]
        owned[B.pay_off[i]:B.pay_off[i] + len(w)] = True
    if B.n - 1 not in skip:
        assert int(o[B.n]) == B.pay_off[-1] + len(want[-1])
    assert np.all(got[~owned] == SENT)


@pytest.mark.parametrize("V", VS)
def test_pack_equals_restatement(ctx, B, V):
    out, poff, pbytes, _ = run_pack(ctx, B, V)
    check_packed(B, V, out, poff, pbytes)


@pytest.mark.parametrize("V", VS)
def test_unpack_round_trip(ctx, B, V):
    """wc_unpack of the device's own packed slots: the source bytes at V = 4, the
    restatement's quantised payload at V = 2, 3; packing that again gives the same
    packed bytes."""
    out, poff, pbytes, _ = run_pack(ctx, B, V)
    pay, off, kept = run_unpack(ctx, B, out, poff, B.slots[V][1])
    check_unpacked(B, B.quant[V], pay, off, kept)
    if V == 4:
        check_unpacked(B, B.pays, pay, off, kept)
    again, poff2, pbytes2, _ = run_pack(ctx, B, V, d_pay=pay, d_off=off)
    check_packed(B, V, again, poff2, pbytes2)


@pytest.mark.parametrize("V", VS)
def test_unpack_of_a_dense_layout(ctx, B, V):
    """wc_unpack reads the restatement's units from the dense layout of the host
    form, with packed_capacity exactly the end of the last unit."""
    buf, off, end = B.dense(V)
    pay, o, kept = run_unpack(ctx, B, dev(buf), u64(off), end)
    check_unpacked(B, B.quant[V], pay, o, kept)


@pytest.mark.parametrize("V", (2, 3))
def test_decoders_read_unpacked_payloads(ctx, wc, BN, V):
    """wc_inverse_levels, wc_inverse (the L = 1 units), wc_inverse_coarse (r = 1) and
    wc_inverse_region (one aligned block) on wc_unpack's output against
    levels_ref, coarse_ref and region_ref on the quantised payload; and the derived
    error bound || decode(q(p)) - decode(p) || <= 2^(s - 24) || decode(p) || on the
    device's cells, per unit, without slack."""
    import torch
    B = BN
    out, poff, pbytes, _ = run_pack(ctx, B, V)
    pay, off, kept = run_unpack(ctx, B, out, poff, B.slots[V][1])
    cells = torch.full((B.extent + 8,), -77.0, dtype=torch.float32, device=pay.device)
    torch.cuda.synchronize()
    ctx.inverse_levels(pay.data_ptr(), off.data_ptr(), B.units, B.n, B.levels, cells.data_ptr())
    ctx.synchronize()
    got = cells.cpu().numpy()
    for i, (W, H, D) in enumerate(B.dims):
        o = B.units[i].cell_offset
        want = LR.decode(B.quant[V][i])[0]
        mine = got[o:o + W * H * D].reshape(D, H, W)
        assert mine.tobytes() == want.tobytes(), (B.what[i], V)
        ref = LR.decode(B.pays[i])[0].astype(np.float64)
        err = float(np.sqrt(np.sum((mine.astype(np.float64) - ref) ** 2)))
        bound = 2.0 ** (8 * (4 - V) - 24) * float(np.sqrt(np.sum(ref ** 2)))
        assert err <= bound, (B.what[i], V, err, bound)
    # the one-level units through wc_inverse
    one = [i for i in range(B.n) if B.levels[i] == 1]
    S = Batch(wc, [(B.what[i], B.pays[i], True) for i in one])
    o1, p1, _, _ = run_pack(ctx, S, V)
    pay1, off1, _ = run_unpack(ctx, S, o1, p1, S.slots[V][1])
    cells1 = torch.full((S.extent + 8,), -77.0, dtype=torch.float32, device=pay.device)
    torch.cuda.synchronize()
    ctx.inverse(pay1.data_ptr(), off1.data_ptr(), S.units, S.n, cells1.data_ptr())
    ctx.synchronize()
    got1 = cells1.cpu().numpy()
    for i, (W, H, D) in enumerate(S.dims):
        o = S.units[i].cell_offset
        assert got1[o:o + W * H * D].tobytes() == LR.decode(S.quant[V][i])[0].tobytes(), S.what[i]
    # r = 1
    cu, cext = wc.capi.coarse_units(B.units, B.n, 1)
    cc = torch.full((cext + 8,), -77.0, dtype=torch.float32, device=pay.device)
    torch.cuda.synchronize()
    ctx.inverse_coarse(pay.data_ptr(), off.data_ptr(), B.units, B.n, B.levels, 1, cu, cc.data_ptr())
    ctx.synchronize()
    gotc = cc.cpu().numpy()
    for i, (W, H, D) in enumerate(B.dims):
        w, h, d = W >> 1, H >> 1, D >> 1
        o = cu[i].cell_offset
        assert gotc[o:o + w * h * d].tobytes() == CR.decode(B.quant[V][i], 1).tobytes(), (B.what[i], V)
    # one aligned block per unit: the second 2^L-cube along x
    regions = [((1 << L) if W >= (2 << L) else 0, 0, 0, 1 << L, 1 << L, 1 << L) if W * H * D else (0,) * 6
               for (W, H, D), L in zip(B.dims, B.levels)]
    ru, rext = wc.capi.region_units(B.units, B.n, regions)
    rc = torch.full((rext + 8,), -77.0, dtype=torch.float32, device=pay.device)
    torch.cuda.synchronize()
    ctx.inverse_region(pay.data_ptr(), off.data_ptr(), B.units, B.n, B.levels, None, regions, ru, rc.data_ptr())
    ctx.synchronize()
    gotr = rc.cpu().numpy()
    for i, g in enumerate(regions):
        o = ru[i].cell_offset
        assert gotr[o:o + g[3] * g[4] * g[5]].tobytes() == RR.decode(B.quant[V][i], 0, g).tobytes(), (B.what[i], V)


def test_existing_decoder_refuses_a_packed_unit(ctx, wc, BN):
    import torch
    one = [i for i in range(BN.n) if BN.levels[i] == 1 and BN.dims[i][2]]
    S = Batch(wc, [(BN.what[i], BN.pays[i], True) for i in one])
    out, poff, _, _ = run_pack(ctx, S, 3)
    cells = torch.full((S.extent + 8,), -77.0, dtype=torch.float32, device=out.device)
    torch.cuda.synchronize()
    ctx.inverse(out.data_ptr(), poff.data_ptr(), S.units, S.n, cells.data_ptr())
    with pytest.raises(wc.WaveletError) as e:
        ctx.synchronize()
    assert e.value.code == wc.capi.WC_ERR_FORMAT


@functools.lru_cache(maxsize=None)
def by_name():
    return {w: p for w, p, _ in PR.batch("f32")}


def small(wc, mid):
    """[a good unit, `mid`, a good unit]."""
    by = by_name()
    return Batch(wc, [("n63", by["n63"], True), ("mid", mid, False), ("n65", by["n65"], True)])


def std(n, runs=None, W=8, H=8, D=8, L=1):
    runs = np.arange(n, dtype=np.uint32) % 5 if runs is None else np.asarray(runs, np.uint32)
    return PR.standard(W, H, D, L, runs, np.arange(n, dtype=np.uint32) * 977 + 0x3F800000)


# why: (a good payload of the unit, the bytes the call finds in its slot instead)
PACK_REFUSALS = {
    "negative_run": lambda: (std(70), std(70, np.where(np.arange(70) == 66, 0x80000005, 3))),
    "nrle_above_cells": lambda: (std(8, W=2, H=2, D=2), std(9, W=2, H=2, D=2)[:84]),  # the ninth pair is never read
    "not_a_header": lambda: (std(70), std(70)[:12] + np.array([-5], np.int32).tobytes() + std(70)[16:]),
    "other_dims": lambda: (std(70), std(70, W=4, H=8, D=16)),
    "already_packed": lambda: (std(70), PR.pack(std(70), 3)),
}


@pytest.mark.parametrize("why", list(PACK_REFUSALS))
def test_pack_refuses_on_the_device(ctx, wc, why):
    """A refused source unit raises WC_ERR_FORMAT at wc_synchronize; the other units
    are packed, and nothing is written outside the refused unit's slot."""
    good, bad = PACK_REFUSALS[why]()
    B = small(wc, good)
    buf = B.buf.copy()
    o = B.pay_off[1]
    assert len(bad) <= B.pay_off[2] - o - 4
    buf[o:o + len(bad)] = np.frombuffer(bad, np.uint8)
    out, poff, pbytes, _ = run_pack(ctx, B, 3, d_pay=dev(buf), sync=False)
    with pytest.raises(wc.WaveletError) as e:
        ctx.synchronize()
    assert e.value.code == wc.capi.WC_ERR_FORMAT
    check_packed(B, 3, out, poff, pbytes, skip=(1,))
    if why != "negative_run":  # a refused header writes nothing at all
        s = B.slots[3][0]
        assert np.all(host(out)[s[1]:s[2]] == SENT) and int(host(pbytes, np.uint64)[1]) == 0
    ctx.synchronize()  # the error word was cleared


def unpack_refusals(B, V=3):
    buf, off, end = B.dense(V)
    o = off[1]

    def tagged(t):
        b = buf.copy()
        b[o + 12:o + 16] = np.frombuffer(np.array([t], np.int32).tobytes(), np.uint8)
        return b, off, end

    def table(v):
        b = buf.copy()
        b[o + 20] = v
        return b, off, end

    def nrle(v):
        b = buf.copy()
        b[o + 16:o + 20] = np.frombuffer(np.array([v], np.int32).tobytes(), np.uint8)
        return b, off, end

    def moved():
        return buf, [off[0], off[1] + 4, off[2]], end

    return {"standard_tag": lambda: tagged(512), "tag_below": lambda: tagged(-69), "tag_levels": lambda: tagged(-(16 * 3 + 5)),
            "width_32": lambda: table(32), "width_255": lambda: table(255), "nrle_above_cells": lambda: nrle(513),
            "nrle_negative": lambda: nrle(-1), "offset_0_mod_8": moved}


@pytest.mark.parametrize("why", ["standard_tag", "tag_below", "tag_levels", "width_32", "width_255", "nrle_above_cells",
                                 "nrle_negative", "offset_0_mod_8"])
def test_unpack_refuses_on_the_device(ctx, wc, why):
    B = small(wc, std(70))
    buf, off, end = unpack_refusals(B)[why]()
    pay, o, kept = run_unpack(ctx, B, dev(buf), u64(off), end, sync=False)
    with pytest.raises(wc.WaveletError) as e:
        ctx.synchronize()
    assert e.value.code == wc.capi.WC_ERR_FORMAT
    check_unpacked(B, B.quant[3], pay, o, kept, skip=(1,))
    ctx.synchronize()


@pytest.mark.parametrize("cut", [1, 9, 200, "table", "header"])
def test_unpack_stops_at_the_capacity(ctx, wc, cut):
    """A unit whose length from header and table would pass packed_capacity is
    refused, and nothing at or past the capacity is read: the buffer ends there."""
    by = by_name()
    B = Batch(wc, [("n63", by["n63"], True), ("n65", by["n65"], True), ("bad", std(300), False)])
    buf, off, end = B.dense(3)
    n_cut = {"table": end - (off[2] + 20 + 4), "header": end - (off[2] + 12)}.get(cut, cut)
    cap = end - n_cut
    pay, o, kept = run_unpack(ctx, B, dev(buf[:cap]), u64(off), cap, sync=False)
    with pytest.raises(wc.WaveletError) as e:
        ctx.synchronize()
    assert e.value.code == wc.capi.WC_ERR_FORMAT
    check_unpacked(B, B.quant[3], pay, o, kept, skip=(2,))


def test_argument_refusals_leave_outputs_untouched(ctx, wc):
    B = small(wc, std(70))
    V = 3
    cap = B.slots[V][1]
    d_pay, d_off = dev(B.buf), u64(B.pay_off)
    out, poff, pbytes = filled(cap + 64), filled(8 * (B.n + 1)), filled(8 * B.n)
    p = dict(pay=d_pay.data_ptr(), off=d_off.data_ptr(), out=out.data_ptr(), poff=poff.data_ptr(), pb=pbytes.data_ptr())

    def pack(V=V, cap=cap, **kw):
        a = dict(p, **kw)
        with pytest.raises(wc.WaveletError) as e:
            ctx.pack(a["pay"], a["off"], B.units, B.n, V, a["out"], cap, a["poff"], a["pb"])
        assert e.value.code == wc.capi.WC_ERR_INVALID

    pack(V=1), pack(V=5), pack(cap=cap - 1), pack(pay=0), pack(off=0), pack(out=0), pack(poff=0), pack(pb=0)
    big, nb, _ = wc.capi.make_units([(128, 128, 129)])
    with pytest.raises(wc.WaveletError) as e:
        ctx.pack(p["pay"], p["off"], big, nb, 3, p["out"], 1 << 40, p["poff"], p["pb"])
    assert e.value.code == wc.capi.WC_ERR_INVALID
    ctx.synchronize()
    for t in (out, poff, pbytes):
        assert np.all(host(t) == SENT)
    buf, off, end = B.dense(V)
    d_pk, d_po = dev(buf), u64(off)
    pay, o, kept = filled(B.pay_cap + 64), filled(8 * (B.n + 1)), filled(4 * B.n)
    q = dict(pk=d_pk.data_ptr(), po=d_po.data_ptr(), pay=pay.data_ptr(), o=o.data_ptr(), k=kept.data_ptr())

    def unpack(cap=B.pay_cap, **kw):
        a = dict(q, **kw)
        with pytest.raises(wc.WaveletError) as e:
            ctx.unpack(a["pk"], a["po"], end, B.units, B.n, a["pay"], cap, a["o"], a["k"])
        assert e.value.code == wc.capi.WC_ERR_INVALID

    unpack(cap=B.pay_cap - 1), unpack(pk=0), unpack(po=0), unpack(pay=0), unpack(o=0), unpack(k=0)
    ctx.synchronize()
    for t in (pay, o, kept):
        assert np.all(host(t) == SENT)


@pytest.mark.parametrize("V", VS)
def test_host_forms_equal_the_device(ctx, wc, B, V):
    packed, poff, pbytes = ctx.pack_host(B.buf, np.asarray(B.pay_off, np.uint64), B.units, B.n, V)
    dense, off, end = B.dense(V)
    assert poff.tolist() == off + [end] and pbytes.tolist() == [len(p) for p in B.packed[V]]
    assert packed.size == end
    for i, want in enumerate(B.packed[V]):
        assert packed[off[i]:off[i] + len(want)].tobytes() == want, (B.what[i], V)
    pay, o, kept = ctx.unpack_host(packed, poff[:B.n], B.units, B.n)
    for i, want in enumerate(B.quant[V]):
        assert wc.capi.unit_payload(pay, o, kept, i) == want, (B.what[i], V)
    # a refused unit fails the host call
    bad = packed.copy()
    bad[off[1] + 12:off[1] + 16] = np.frombuffer(np.array([-70], np.int32).tobytes(), np.uint8)
    with pytest.raises(wc.WaveletError) as e:
        ctx.unpack_host(bad, poff[:B.n], B.units, B.n)
    assert e.value.code == wc.capi.WC_ERR_FORMAT


def test_codec_round_trips(wc, BN, tmp_path):
    """codec.compress_payloads(pack=) returns the restatement's packed units, after
    the keep rule and after levels=; decompress_payloads reads packed units, a
    mixed list, coarsen = 1 and a region; compress(pack=) / decompress through a file."""
    from tol_rule import field
    codec = wc.codec
    boxes = [field(0, 16, 16, 16, 9200), field(2, 32, 16, 8, 9201), field(1, 8, 8, 8, 9202)]
    for levels in (1, 2):
        plain = codec.compress_payloads(boxes, 0.99, levels=levels)
        assert [wc.capi.payload_packed(p) for p in plain] == [(levels, 0)] * 3
        for V in VS:
            packed = codec.compress_payloads(boxes, 0.99, levels=levels, pack=V)
            assert packed == [PR.pack(p, V) for p in plain], (levels, V)
            quant = [PR.quantise(p, V) for p in plain]
            assert [wc.capi.payload_packed(p) for p in packed] == [(levels, V)] * 3
            for got, q in zip(codec.decompress_payloads(packed), quant):
                assert got.tobytes() == LR.decode(q)[0].tobytes()
            mixed = [packed[0], plain[1], packed[2]]
            for got, q in zip(codec.decompress_payloads(mixed), [quant[0], plain[1], quant[2]]):
                assert got.tobytes() == LR.decode(q)[0].tobytes()
            for got, q in zip(codec.decompress_payloads(packed, coarsen=1), quant):
                assert got.tobytes() == CR.decode(q, 1).tobytes()
            reg = ((2, 4, 1), (7, 8, 6))
            for got, q in zip(codec.decompress_payloads(mixed, region=reg), [quant[0], plain[1], quant[2]]):
                assert got.tobytes() == LR.decode(q)[0][1:6, 4:8, 2:7].tobytes()
    rm = codec.compress_payloads(boxes, 0.0, levels=2, rmse=0.05, pack=3)
    assert rm == [PR.pack(p, 3) for p in codec.compress_payloads(boxes, 0.0, levels=2, rmse=0.05)]
    bud = codec.compress_payloads(boxes, 0.0, max_bytes=1020, pack=2)
    assert bud == [PR.pack(p, 2) for p in codec.compress_payloads(boxes, 0.0, max_bytes=1020)]
    with pytest.raises(ValueError):
        codec.compress_payloads(boxes, 0.99, pack=5)
    codec.compress(boxes[:2], [3, 7], 0.99, 1, 0, 5, tmp_path, levels=2, pack=3)
    for c, p in zip((3, 7), codec.compress_payloads(boxes[:2], 0.99, levels=2)):
        name = tmp_path / f"compressed-wavelet-1-0-{c}-5.xz"
        assert codec.read_compressed_payload(name) == PR.pack(p, 3)
        assert codec.decompress(name).tobytes() == LR.decode(PR.quantise(p, 3))[0].tobytes()


def test_caller_stream_without_a_host_sync(wc, B):
    """On a torch stream s after wc_set_stream(s): a delay, the producer (the copy
    of the payloads into a zeroed buffer), wc_pack, wc_unpack of its slots, clones
    of the outputs and their overwrite, all enqueued without a host sync.  After
    s.synchronize() alone the clones hold the restatement's bytes."""
    import torch
    V = 3
    ctx = wc.capi.Context(0)
    s = torch.cuda.Stream()
    try:
        real, d_off = dev(B.buf), u64(B.pay_off)
        src = real.clone()
        cap = B.slots[V][1]
        out, poff, pbytes = filled(cap + 64), filled(8 * (B.n + 1)), filled(8 * B.n)
        pay, off, kept = filled(B.pay_cap + 64), filled(8 * (B.n + 1)), filled(4 * B.n)

        def enqueue():
            ctx.pack(src.data_ptr(), d_off.data_ptr(), B.units, B.n, V, out.data_ptr(), cap, poff.data_ptr(),
                     pbytes.data_ptr())
            ctx.unpack(out.data_ptr(), poff.data_ptr(), cap, B.units, B.n, pay.data_ptr(), B.pay_cap, off.data_ptr(),
                       kept.data_ptr())

        enqueue()  # once with plain syncs: the descriptors are uploaded, nothing afterwards allocates
        ctx.synchronize()
        with torch.cuda.stream(s):
            spare = [t.clone() for t in (out, poff, pbytes, pay, off, kept)]
        s.synchronize()
        del spare
        for t in (out, poff, pbytes, pay, off, kept):
            t.fill_(SENT)
        src.zero_()
        torch.cuda.synchronize()
        ctx.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            torch.cuda._sleep(100_000_000)
            src.copy_(real)
            enqueue()
            c = [t.clone() for t in (out, poff, pbytes, pay, off, kept)]
            for t in (out, poff, pbytes, pay, off, kept):
                t.fill_(0)
            src.fill_(0xFF)
            busy = not s.query()
        assert busy, "the stream was idle right after the last enqueue: a call blocked, so this test had no power"
        s.synchronize()
        check_packed(B, V, c[0], c[1], c[2])
        check_unpacked(B, B.quant[V], c[3], c[4], c[5])
        ctx.synchronize()
    finally:
        ctx.set_stream(None)
        ctx.close()


def test_profile_books_the_pack_stage(ctx, B):
    ctx.profile_enable(True)
    try:
        ctx.profile_read()
        out, poff, pbytes, _ = run_pack(ctx, B, 3)
        run_unpack(ctx, B, out, poff, B.slots[3][1])
        prof = ctx.profile_read()
        assert set(prof) == {"pack"} and prof["pack"][1] == 2 and prof["pack"][0] > 0.0
    finally:
        ctx.profile_enable(False)
