"""GPU: the decoders over packed units (include/wavelet_amd.h wc_inverse_packed,
wc_inverse_packed_coarse, wc_inverse_packed_region and their _host forms;
codec.decompress_payloads on packed payloads).

Bar: bit for bit what wc_unpack followed by wc_inverse_levels / wc_inverse_coarse
/ wc_inverse_region gives on the same units, whole output buffers compared, the
sentinel between the units included.  Against the CPU restatements (levels_ref,
coarse_ref, region_ref on the quantised payload) the existing same_cells rule:
on the field batch at every V, on the crafted corpus at V = 4, where the
quantised payload is the source (at V = 2, 3 the twin is the yardstick there, and
tests/test_gpu_pack.py holds the twin to the restatements).

Before every packed call the same units decode from all-kept standard payloads,
so that a tile that never runs leaves stale coefficients, not the right ones.

Corpus: pack_rule.batch's field units (L = 1..3, 0..2049 pairs, a unit without
cells, all-zero widths, the 64^3 unit) and the packable crafted units
(tests/packed_decode_ref.corpus, checked in tests/test_packed_decode_cpu.py)."""
import functools

import numpy as np
import pytest

import coarse_ref as C
import decode_payloads as DP
import levels_ref as LR
import pack_rule as PR
import packed_decode_ref as R
import region_ref as G
from test_gpu_fuzz import same_cells

pytestmark = pytest.mark.gpu

SENT = -77.0
VS = (2, 3, 4)
BATCH = 60
_REF = {}  # (payload bytes, kind, r, region) -> reference cells, computed once and left unchanged


def reference(pay, kind, r, region):
    key = (pay, kind, r, region)
    if key not in _REF:
        W, H, D = (int(v) for v in np.frombuffer(pay[:12], np.int32))
        if W * H * D == 0 or (kind == "region" and region[3] * region[4] * region[5] == 0):
            _REF[key] = np.zeros(0, np.float32)
        elif kind == "levels":
            _REF[key] = LR.decode(pay)[0]
        elif kind == "coarse":
            _REF[key] = C.decode(pay, r)
        else:
            _REF[key] = G.decode(pay, r, region)
        _REF[key].flags.writeable = False
    return _REF[key]


@functools.lru_cache(maxsize=None)
def packed_of(pay, V):
    return PR.pack(pay, V)


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def filled_bytes(nbytes):
    import torch
    t = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def fresh(extent):
    import torch
    t = torch.full((extent,), SENT, dtype=torch.float32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()  # the fill runs on torch's stream, the context on its own
    return t


class Entries:
    """One call: entries (standard payload, r, region or None) packed at V, the
    packed units in the slot layout of wc_pack or the dense layout of
    wc_pack_host (the buffer then ends at the last unit's last byte), the output
    units with gaps and odd offsets."""

    def __init__(self, wc, entries, kind, V, layout="slots", seed=0):
        rng = np.random.default_rng(8800 + seed)
        self.kind, self.V, self.n = kind, V, len(entries)
        self.pays = [p for p, _, _ in entries]
        self.dims = [tuple(int(v) for v in np.frombuffer(p[:12], np.int32)) for p in self.pays]
        self.cells = [w * h * d for w, h, d in self.dims]
        self.levels = [PR.parse(p)[3] for p in self.pays]
        self.reduce = [r for _, r, _ in entries]
        self.regions = [((0, 0, 0) + dm if g is None else tuple(g)) if c else (0, 0, 0, 0, 0, 0)
                        for (_, _, g), dm, c in zip(entries, self.dims, self.cells)]
        self.cdims = self.dims if kind == "levels" else [G.out_dims(g, r) for g, r in zip(self.regions, self.reduce)]
        self.offs, self.extent = DP.cell_layout([w * h * d for w, h, d in self.cdims], rng)
        self.out_units, _, _ = wc.capi.make_units(self.cdims, self.offs)
        self.units = self.out_units if kind == "levels" else wc.capi.make_units(self.dims)[0]
        self.packed = [packed_of(p, V) for p in self.pays]
        self.place(layout)
        self.pay_off, self.pay_cap = PR.payload_slots(self.dims)
        self.owned = np.zeros(self.extent, bool)
        for o, (w, h, d) in zip(self.offs, self.cdims):
            self.owned[o:o + w * h * d] = True

    def place(self, layout, packed=None, order=None):
        """The packed buffer: offsets, the capacity, the bytes (the gaps hold no header)."""
        packed = self.packed if packed is None else packed
        if layout == "slots":
            off, cap = PR.slot_offsets(self.dims, self.V)
        else:
            off, cur = [0] * self.n, 4
            for i in (range(self.n) if order is None else order):
                off[i] = cur
                cur += PR.pad8(len(packed[i]))
                cap = off[i] + len(packed[i])
        self.buf = np.full(cap + (64 if layout == "slots" else 0), 0xA5, np.uint8)
        for o, p in zip(off, packed):
            self.buf[o:o + len(p)] = np.frombuffer(p, np.uint8)
        self.poff, self.cap = np.array(off + [0], np.uint64)[:max(self.n, 1)], cap

    def want(self, i):
        """The CPU restatement's cells of entry i, on the quantised payload."""
        g = self.regions[i] if self.kind == "region" else None
        return reference(PR.quantise(self.pays[i], self.V), self.kind, self.reduce[i], g)

    def dirty(self):
        """All-kept standard payloads of the same units (every coefficient 7.5), in the forward's slots."""
        buf = np.zeros(self.pay_cap + 8, np.uint8)
        for o, dm, L, c in zip(self.pay_off, self.dims, self.levels, self.cells):
            p = PR.standard(*dm, L, np.zeros(c, np.uint32), np.full(c, 0x40F00000, np.uint32))
            buf[o:o + len(p)] = np.frombuffer(p, np.uint8)
        return buf, np.array(self.pay_off + [0], np.uint64)[:max(self.n, 1)]


def standard_call(ctx, E, pay, off, out):
    if E.kind == "levels":
        ctx.inverse_levels(pay, off, E.units, E.n, E.levels, out)
    elif E.kind == "coarse":
        ctx.inverse_coarse(pay, off, E.units, E.n, E.levels, E.reduce, E.out_units, out)
    else:
        ctx.inverse_region(pay, off, E.units, E.n, E.levels, E.reduce, E.regions, E.out_units, out)


def packed_call(ctx, E, pk, off, cap, out):
    if E.kind == "levels":
        ctx.inverse_packed(pk, off, cap, E.units, E.n, E.levels, out)
    elif E.kind == "coarse":
        ctx.inverse_packed_coarse(pk, off, cap, E.units, E.n, E.levels, E.reduce, E.out_units, out)
    else:
        ctx.inverse_packed_region(pk, off, cap, E.units, E.n, E.levels, E.reduce, E.regions, E.out_units, out)


def twin(ctx, E, d_pk, d_off):
    """wc_unpack + the standard call -> the whole output buffer."""
    pay, off, kept = filled_bytes(E.pay_cap + 64), filled_bytes(8 * (E.n + 1)), filled_bytes(4 * max(E.n, 1))
    out = fresh(E.extent)
    ctx.unpack(d_pk.data_ptr(), d_off.data_ptr(), E.cap, E.units, E.n, pay.data_ptr(), E.pay_cap, off.data_ptr(),
               kept.data_ptr())
    standard_call(ctx, E, pay.data_ptr(), off.data_ptr(), out.data_ptr())
    ctx.synchronize()
    return out.cpu().numpy()


def direct(ctx, E, d_pk, d_off, dirty=True):
    """The packed call into a sentinel-filled buffer, after a decode that dirties the scratch."""
    if dirty:
        buf, off = E.dirty()
        d_buf, d_o = dev(buf), dev(off)
        scratch = fresh(E.extent)
        standard_call(ctx, E, d_buf.data_ptr(), d_o.data_ptr(), scratch.data_ptr())
    out = fresh(E.extent)
    packed_call(ctx, E, d_pk.data_ptr(), d_off.data_ptr(), E.cap, out.data_ptr())
    ctx.synchronize()
    return out.cpu().numpy()


def identical(a, b):
    return a.view(np.uint32).tobytes() == b.view(np.uint32).tobytes()


def check_identity(ctx, E, what, restated):
    d_pk, d_off = dev(E.buf), dev(E.poff)
    got = direct(ctx, E, d_pk, d_off)
    ref = twin(ctx, E, d_pk, d_off)
    assert np.all(got[~E.owned] == SENT), what  # nothing outside a unit's cells
    if not identical(got, ref):
        for i in range(E.n):
            o, c = E.offs[i], int(np.prod(E.cdims[i]))
            assert identical(got[o:o + c], ref[o:o + c]), (what, i, E.dims[i], E.levels[i], E.reduce[i], E.regions[i])
        raise AssertionError(what)
    if restated:
        for i in range(E.n):
            w = E.want(i)
            assert same_cells(got[E.offs[i]:E.offs[i] + w.size], w.ravel()), (what, "restatement", i)
    assert d_pk.cpu().numpy().tobytes() == E.buf.tobytes(), what  # the source is only read
    return got


def chunks(items, size=BATCH):
    return [items[a:a + size] for a in range(0, len(items), size)]


def aligned(dims, L):
    return dims[0] * dims[1] * dims[2] > 0 and (dims[0] | dims[1] | dims[2]) & ((1 << L) - 1) == 0


def modes_of(pay):
    """(kind, r, region) a payload is decoded under: the full decode; every r <= L; the regions
    decode_payloads.regions_of gives (the whole box, a slab per axis, one block) at r = 0 and 1, and an empty one."""
    W, H, D, L, _, _ = PR.parse(pay)
    out = [("levels", 0, None)]
    if aligned((W, H, D), L):
        out += [("coarse", r, None) for r in range(L + 1)]
        out += [("region", r, g) for r in (0, 1) for g in DP.regions_of((W, H, D), L)]
        out.append(("region", 0, (0, 0, 0, 0, 0, 0)))
    return out


# ------------------------------------------------------------------ identity --
@functools.lru_cache(maxsize=None)
def field_units():
    return tuple(p for _, p, fin in PR.batch("f32") if fin)


@pytest.mark.parametrize("layout", ("slots", "dense"))
@pytest.mark.parametrize("V", VS)
def test_field_batch(wc, ctx, V, layout):
    """The field batch of test_gpu_pack.py through the three calls, in both layouts
    (dense: packed_capacity is the last unit's last byte), against the twins and the restatements."""
    pays = field_units()
    for kind in ("levels", "coarse", "region"):
        entries = [(p, r, g) for p in pays for k, r, g in modes_of(p) if k == kind]
        E = Entries(wc, entries, kind, V, layout, seed=V)
        assert layout == "slots" or E.buf.size == E.cap
        check_identity(ctx, E, ("field", kind, V, layout), restated=True)


CORPUS = R.corpus()
LEVELS = chunks([(u, 0, None) for u in CORPUS])
CUBES = [u for u in CORPUS if u.dims == DP.CUBE]
COARSE = chunks([(u, r, None) for u in CUBES for r in range(u.L + 1)])
REGION = chunks([(u, r, g) for u in CUBES for r in (0, 1) for g in DP.regions_of(DP.CUBE, u.L)])


def corpus_case(wc, ctx, part, kind, k, V):
    E = Entries(wc, [(u.payload, r, g) for u, r, g in part[k]], kind, V, "dense" if (k + V) % 2 else "slots", seed=10 * k + V)
    check_identity(ctx, E, ("corpus", kind, k, V), restated=V == 4)


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("k", range(len(LEVELS)))
def test_corpus_full(wc, ctx, k, V):
    corpus_case(wc, ctx, LEVELS, "levels", k, V)


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("k", range(len(COARSE)))
def test_corpus_coarse(wc, ctx, k, V):
    corpus_case(wc, ctx, COARSE, "coarse", k, V)


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("k", range(len(REGION)))
def test_corpus_region(wc, ctx, k, V):
    corpus_case(wc, ctx, REGION, "region", k, V)


def test_fuzz_widths(wc, ctx):
    """Every chunk width 0..31 and short last chunks on odd boxes (pack_rule.fuzz_batch): the full decode
    against the twin; these units' runs need not fit their boxes."""
    for seed in PR.FUZZ_SEEDS:
        E = Entries(wc, [(p, 0, None) for _, p, _ in PR.fuzz_batch(seed)], "levels", 2 + seed % 3, "dense", seed=seed)
        check_identity(ctx, E, ("widths", seed), restated=False)


# ------------------------------------------------------------ look-back forms --
HARD = [u for u in CORPUS if len(u.runs) > DP.TILE and (u.cls.startswith("ov:") or u.cls == "n=8193" or u.dims == DP.CUBE)][:BATCH]
_OPTION_SETS = {
    "ordered_0": (("WC_OPT_ORDERED", 0),),
    "ordered_1": (("WC_OPT_ORDERED", 1),),
    "reversed_tiles": (("WC_OPT_REVERSE_TILES", 1),),
    "spin_limit_1": (("WC_OPT_SPIN_LIMIT", 1),),
    "reversed_spin_1": (("WC_OPT_REVERSE_TILES", 1), ("WC_OPT_SPIN_LIMIT", 1)),
    "tickets_spin_1": (("WC_OPT_ORDERED", 0), ("WC_OPT_SPIN_LIMIT", 1)),
}


@pytest.mark.parametrize("kind", ("levels", "coarse", "region"))
def test_lookback_forms(wc, ctx, kind):
    """The multi-tile units (8193 pairs on 32^3, the overshoot classes) under every tile order and with the
    wait bound at 1, where waits take the derive path (PackedPairs::tile_sum): the cells of the default form.
    The options are restored afterwards."""
    assert any(u.cls == "n=8193" and u.dims == DP.CUBE for u in HARD) and any(u.cls == "ov:lookback" for u in HARD)
    units = HARD if kind == "levels" else [u for u in HARD if u.dims == DP.CUBE]
    far = lambda u: DP.regions_of(u.dims, u.L)[4]
    entries = [(u.payload, 0 if kind == "levels" else i % (u.L + 1), far(u) if kind == "region" and i % 2 else None)
               for i, u in enumerate(units)]
    E = Entries(wc, entries, kind, 3, "dense", seed=77)
    d_pk, d_off = dev(E.buf), dev(E.poff)
    ref = twin(ctx, E, d_pk, d_off)
    for name, opts in sorted(_OPTION_SETS.items()):
        keys = [(getattr(wc.capi, o), v) for o, v in opts]
        before = [(k, ctx.get_option(k)) for k, _ in keys]
        for k, v in keys:
            ctx.set_option(k, v)
        try:
            got = direct(ctx, E, d_pk, d_off)
        finally:
            for k, v in before:
                ctx.set_option(k, v)
        assert identical(got, ref), (kind, name)


# ------------------------------------------------------------------ refusals --
def _victim():
    """8193 pairs on 32^3 with runs of 0..3: three pair tiles, 129 chunks, the last of one pair."""
    rng = np.random.default_rng(8801)
    n = 8193
    return PR.standard(32, 32, 32, 1, rng.integers(0, 4, n), DP._finite_bits(rng, n))


def _with(packed, **kw):
    b = bytearray(packed)
    h = np.frombuffer(bytes(b[:20]), np.int32).copy()
    if "tag" in kw:
        h[3] = kw["tag"]
    if "n" in kw:
        h[4] = kw["n"]
    b[:20] = h.tobytes()
    if "width" in kw:
        b[20 + kw["width"]] = 32
    return bytes(b)


V_REF = 3
# name -> (what to do to the victim's packed bytes, header-level: the unit's cells stay untouched)
REFUSALS = {
    "wrong_tag": (lambda p: _with(p, tag=-(16 * 5 + 1)), True),
    "standard_tag": (lambda p: _with(p, tag=32 ** 3), True),
    "wrong_L": (lambda p: _with(p, tag=PR.tag(2, V_REF)), True),
    "n_above_cells": (lambda p: _with(p, n=32 ** 3 + 1), True),
    "width_32_first_tile": (lambda p: _with(p, width=3), False),
    "width_32_middle_tile": (lambda p: _with(p, width=64 + 17), False),
    "width_32_last_tile": (lambda p: _with(p, width=128), False),
    "cut_in_table": ("cut", 20 + 77, True),
    "cut_in_middle_chunk": ("cut", None, False),
    "cut_in_last_chunk": ("cut", -1, False),
    "offset_0_mod_8": ("shift", None, True),
}


@pytest.mark.parametrize("kind", ("levels", "coarse", "region"))
@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals(wc, ctx, kind, case):
    """A refused unit between two good ones (last in the buffer where the capacity is cut): WC_ERR_FORMAT at
    synchronize, the other units bit-exact, the unit's cells untouched for a header-level refusal, and in every
    case no cell outside a unit's output range written."""
    small = PR.standard(16, 16, 16, 1, np.zeros(900, np.uint32), DP._finite_bits(np.random.default_rng(5), 900))
    mode = {"levels": (0, None), "coarse": (1, None), "region": (0, (24, 24, 24, 8, 8, 8))}[kind]
    smode = {"levels": (0, None), "coarse": (1, None), "region": (0, (8, 8, 8, 8, 8, 8))}[kind]
    cube = next(u for u in CORPUS if u.cls == "n=4097" and u.dims == DP.CUBE and u.L == 1)
    entries = [(small,) + smode, (_victim(),) + mode, (cube.payload,) + mode]
    E = Entries(wc, entries, kind, V_REF, "dense", seed=3)
    good = twin(ctx, E, dev(E.buf), dev(E.poff))  # the batch before it is damaged
    spec = REFUSALS[case]
    packed, order = list(E.packed), [0, 2, 1]  # the victim last in the buffer
    if callable(spec[0]):
        packed[1] = spec[0](packed[1])
    E.place("dense", packed, order)
    if spec[0] == "cut":
        o, ln = int(E.poff[1]), len(packed[1])
        E.cap = o + (spec[1] if spec[1] and spec[1] > 0 else ln - 1 if spec[1] == -1 else ln // 2)
        E.buf = E.buf[:E.cap].copy()
    if spec[0] == "shift":  # the victim at an offset that is 0 (mod 8)
        o = int(E.poff[1]) + 4
        E.buf = np.concatenate([E.buf[:int(E.poff[1])], np.full(4, 0xA5, np.uint8), np.frombuffer(packed[1], np.uint8)])
        E.poff[1], E.cap = o, o + len(packed[1])
    out = fresh(E.extent)
    d_pk, d_off = dev(E.buf), dev(E.poff)
    packed_call(ctx, E, d_pk.data_ptr(), d_off.data_ptr(), E.cap, out.data_ptr())
    with pytest.raises(wc.capi.WaveletError) as e:
        ctx.synchronize()
    assert e.value.code == wc.capi.WC_ERR_FORMAT, case
    got = out.cpu().numpy()
    assert np.all(got[~E.owned] == SENT), case
    for i in (0, 2):
        o, c = E.offs[i], int(np.prod(E.cdims[i]))
        assert identical(got[o:o + c], good[o:o + c]), (case, i)
    if spec[-1]:
        o, c = E.offs[1], int(np.prod(E.cdims[1]))
        assert np.all(got[o:o + c] == SENT), case
    ctx.synchronize()  # the error was read and cleared


def test_argument_refusals(wc, ctx):
    """WC_ERR_INVALID before any launch; the outputs stay untouched."""
    cube = next(u for u in CORPUS if u.cls == "n=4097" and u.dims == DP.CUBE and u.L == 2)
    out = fresh(40000)

    def refused(fn):
        with pytest.raises(wc.capi.WaveletError) as e:
            fn()
        assert e.value.code == wc.capi.WC_ERR_INVALID
        ctx.synchronize()
        assert np.all(out.cpu().numpy() == SENT)

    for kind, mode in (("levels", (0, None)), ("coarse", (1, None)), ("region", (1, (0, 0, 0, 8, 8, 8)))):
        E = Entries(wc, [(cube.payload,) + mode], kind, 3, "dense")
        d_pk, d_off = dev(E.buf), dev(E.poff)
        refused(lambda: packed_call(ctx, E, 0, d_off.data_ptr(), E.cap, out.data_ptr()))
        refused(lambda: packed_call(ctx, E, d_pk.data_ptr(), 0, E.cap, out.data_ptr()))
        refused(lambda: packed_call(ctx, E, d_pk.data_ptr(), d_off.data_ptr(), E.cap, 0))
        refused(lambda: packed_call(ctx, E, d_pk.data_ptr() + 4, d_off.data_ptr(), E.cap, out.data_ptr()))  # 8-B aligned, as wc_unpack
        big = wc.capi.make_units([(128, 128, 256)])[0]  # above WC_PACK_MAX_CELLS
        keep = E.units, E.out_units
        E.units = big
        if kind == "levels":
            refused(lambda: packed_call(ctx, E, d_pk.data_ptr(), d_off.data_ptr(), E.cap, out.data_ptr()))
        E.units, E.out_units = keep
        E.levels = [5]
        refused(lambda: packed_call(ctx, E, d_pk.data_ptr(), d_off.data_ptr(), E.cap, out.data_ptr()))
        E.levels = [2]
        if kind != "levels":
            E.reduce = [3]  # above L
            refused(lambda: packed_call(ctx, E, d_pk.data_ptr(), d_off.data_ptr(), E.cap, out.data_ptr()))
            E.reduce = [1]
            E.out_units = wc.capi.make_units([(5, 5, 5)])[0]
            refused(lambda: packed_call(ctx, E, d_pk.data_ptr(), d_off.data_ptr(), E.cap, out.data_ptr()))
        if kind == "region":
            E.out_units = keep[1]
            E.regions = [(2, 0, 0, 8, 8, 8)]  # not aligned to 2^L
            refused(lambda: packed_call(ctx, E, d_pk.data_ptr(), d_off.data_ptr(), E.cap, out.data_ptr()))


def test_output_smaller_than_the_payload_bound(wc, ctx):
    """The memory claim in a form a test can hold: on a batch whose wc_payload_bound exceeds its output many
    times over, the direct calls return the right cells (they allocate nothing of that size; the figure is
    measured by tools/bench_packed_decode.py)."""
    cubes = [u for u in CUBES if u.L == 3 and u.cls.startswith("n=")][:8]
    for kind, mode in (("coarse", (3, None)), ("region", (0, (24, 24, 24, 8, 8, 8)))):
        E = Entries(wc, [(u.payload,) + mode for u in cubes], kind, 2, "dense", seed=9)
        assert wc.capi.payload_bound(E.units, E.n) > 16 * 4 * E.extent
        check_identity(ctx, E, ("bound", kind), restated=False)


# ------------------------------------------------------- host forms, callers --
def host_call(ctx, E, buf, off, out, levels="given"):
    lv = E.levels if levels == "given" else None
    if E.kind == "levels":
        return ctx.inverse_packed_host(buf, off, E.units, E.n, E.extent, levels=lv, out=out)
    if E.kind == "coarse":
        return ctx.inverse_packed_coarse_host(buf, off, E.units, E.n, E.reduce, E.out_units, E.extent, levels=lv, out=out)
    return ctx.inverse_packed_region_host(buf, off, E.units, E.n, E.reduce, E.regions, E.out_units, E.extent, levels=lv,
                                          out=out)


@pytest.mark.parametrize("kind", ("levels", "coarse", "region"))
def test_host_forms(wc, ctx, kind):
    """The host forms in several unit runs equal the device forms; levels = NULL reads the tags; a refused unit
    fails the call (WC_ERR_FORMAT) with the outputs untouched."""
    pays = field_units()
    entries = [(p, r, g) for p in pays for k, r, g in modes_of(p) if k == kind]
    E = Entries(wc, entries, kind, 3, "dense", seed=21)
    want = direct(ctx, E, dev(E.buf), dev(E.poff), dirty=False)
    before = ctx.get_option(wc.capi.WC_OPT_HOST_CHUNK)
    ctx.set_option(wc.capi.WC_OPT_HOST_CHUNK, 1 << 13)
    try:
        for levels in ("given", "tags"):
            buf, off = E.buf.copy(), E.poff.copy()
            got = host_call(ctx, E, buf, off[:E.n], np.full(E.extent, SENT, np.float32), levels)
            assert identical(got, want), (kind, levels)
            assert buf.tobytes() == E.buf.tobytes() and off.tobytes() == E.poff.tobytes()
        bad = E.buf.copy()
        victim = next(i for i, p in enumerate(E.packed) if len(PR.parse(E.pays[i])[4]) > 64)
        bad[int(E.poff[victim]) + 20] = 32  # a width above 31
        out = np.full(E.extent, SENT, np.float32)
        with pytest.raises(wc.capi.WaveletError) as e:
            host_call(ctx, E, bad, E.poff[:E.n], out)
        assert e.value.code == wc.capi.WC_ERR_FORMAT and np.all(out == SENT)
    finally:
        ctx.set_option(wc.capi.WC_OPT_HOST_CHUNK, before)


def test_codec_round_trip_of_a_mixed_list(wc, monkeypatch):
    """decompress_payloads on standard and packed payloads mixed, in list order, with coarsen= and region=:
    the bits of unpack_payloads followed by the standard path; without region= no unit is unpacked."""
    from tol_rule import field
    codec = wc.codec
    boxes = [field(k % 3, *dm, 9700 + k) for k, dm in enumerate([(16, 16, 16), (32, 16, 8), (8, 8, 24), (16, 8, 8)])]
    std = codec.compress_payloads(boxes, 0.9, levels=2)
    mixed = [std[0], codec.pack_payloads([std[1]], 3)[0], codec.pack_payloads([std[2]], 2)[0], std[3]]
    plain = [std[0]] + codec.unpack_payloads([mixed[1]]) + codec.unpack_payloads([mixed[2]]) + [std[3]]
    assert wc.capi.payload_packed(mixed[1])[1] == 3 and wc.capi.payload_packed(plain[1])[1] == 0
    unpack_host = wc.capi.Context.unpack_host
    for kw in ({}, {"coarsen": 1}, {"region": ((1, 2, 3), (7, 8, 8))}, {"coarsen": 1, "region": ((0, 2, 2), (8, 7, 8))}):
        if "region" not in kw:  # the full and the coarse decode read the packed bytes: nothing is unpacked
            monkeypatch.setattr(wc.capi.Context, "unpack_host", None)
        got = codec.decompress_payloads(mixed, **kw)
        monkeypatch.setattr(wc.capi.Context, "unpack_host", unpack_host)
        want = codec.decompress_payloads(plain, **kw)
        assert len(got) == 4
        for g, w in zip(got, want):
            assert g.shape == w.shape and identical(np.ascontiguousarray(g), np.ascontiguousarray(w)), kw
    only = codec.decompress_payloads(mixed[1:3])  # packed alone: one call
    assert identical(only[0], codec.decompress_payloads(plain[1:2])[0])


def test_caller_stream_without_a_host_sync(wc):
    """On a torch stream s after wc_set_stream(s): a delay, the producer (the copy of the packed units into a
    zeroed buffer), the three packed calls, clones of the outputs and their overwrite, all enqueued without a
    host sync.  After s.synchronize() alone the clones hold the cells of the synchronous run."""
    import torch
    pays = field_units()
    ctx = wc.capi.Context(0)
    s = torch.cuda.Stream()
    try:
        Es = [Entries(wc, [(p, r, g) for p in pays for k, r, g in modes_of(p) if k == kind][:12], kind, 3, "dense", seed=31)
              for kind in ("levels", "coarse", "region")]
        real = [dev(E.buf) for E in Es]
        offs = [dev(E.poff) for E in Es]
        src = [t.clone() for t in real]
        outs = [fresh(E.extent) for E in Es]

        def enqueue():
            for E, p, o, out in zip(Es, src, offs, outs):
                packed_call(ctx, E, p.data_ptr(), o.data_ptr(), E.cap, out.data_ptr())

        enqueue()  # once with plain syncs: plans and descriptors are uploaded, nothing afterwards allocates
        ctx.synchronize()
        want = [t.cpu().numpy() for t in outs]
        with torch.cuda.stream(s):
            spare = [t.clone() for t in outs]
        s.synchronize()
        del spare
        for t in outs:
            t.fill_(SENT)
        for t in src:
            t.zero_()
        torch.cuda.synchronize()
        ctx.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            torch.cuda._sleep(100_000_000)
            for t, r in zip(src, real):
                t.copy_(r)
            enqueue()
            c = [t.clone() for t in outs]
            for t in outs:
                t.fill_(0)
            for t in src:
                t.fill_(0xFF)
            busy = not s.query()
        assert busy, "the stream was idle right after the last enqueue: a call blocked, so this test had no power"
        s.synchronize()
        for got, w in zip(c, want):
            assert identical(got.cpu().numpy(), w)
        ctx.synchronize()
    finally:
        ctx.set_stream(None)
        ctx.close()
