"""GPU: the packed payload transcoders (wc_pack, wc_unpack, wc_pack_host,
wc_unpack_host) on generated units and at their size limits, against the numpy
restatement tests/pack_rule.py.  tests/test_gpu_pack.py holds the fixed batch
and the refusals; its helpers and its bar are used here unchanged: byte for
byte, sentinels outside every exact length.

What each test reaches that the fixed batch does not:
  fuzz          odd dimensions and cell counts, every chunk width 0..31 as a full
                and as a short last chunk, every m % 8 of a last chunk, slots
                filled to S(N) exactly (tests/test_pack_cpu.py proves the
                generator gives these)
  many units    k_dense_offsets past one wave (64, 65 units) and past one pass
                (1024, 1025, 2100 units), both template forms
  the limit     one unit of WC_PACK_MAX_CELLS = 2^21 cells, all kept: 1024 tiles,
                16 passes of block_table_sum over a 32-KiB table; and 100 pairs on
                the same descriptors: 1023 workgroups leave after the header
  layouts       source and packed offsets in another order, with gaps, at 0 and
                at 4 (mod 8), the lowest not unit 0's
  the cache     new batches of the same and of another unit count and a return to
                the first, with the earlier transcodes still in flight
  the pipeline  wc_forward_levels -> wc_pack -> wc_unpack -> wc_inverse_levels
                without a host sync, on the context's stream and on a caller's
"""
import functools
import types

import numpy as np
import pytest

import levels_ref as LR
import pack_rule as PR
from test_gpu_pack import SENT, VS, Batch, check_packed, check_unpacked, dev, filled, host, run_pack, run_unpack, u64
from tol_rule import field

pytestmark = pytest.mark.gpu

MANY = (64, 65, 1024, 1025, 2100)
KEEP = 0.99


@functools.lru_cache(maxsize=None)
def fuzz(wc, seed):
    return Batch(wc, PR.fuzz_batch(seed))


@pytest.fixture(scope="module", params=PR.FUZZ_SEEDS)
def F(request, wc):
    return fuzz(wc, request.param)


@pytest.fixture(scope="module")
def F0(wc):
    return fuzz(wc, PR.FUZZ_SEEDS[0])


@pytest.fixture(scope="module")
def F1(wc):
    return fuzz(wc, PR.FUZZ_SEEDS[1])


@pytest.fixture(scope="module")
def M(wc):
    """many_units(2100) at V = 3; the tests take prefixes of it."""
    return Batch(wc, PR.many_units(max(MANY)), vs=(3,))


@pytest.fixture(scope="module")
def LIMIT(wc):
    """The 2^21-cell unit with all pairs and with 100, restated once, at V = 3 only."""
    return Batch(wc, [PR.limit_unit(2 ** 21)], vs=(3,)), Batch(wc, [PR.limit_unit(100)], vs=(3,))


def check_host_forms(ctx, wc, B, V, buf=None, off=None):
    """wc_pack_host from `buf` / `off` (default: the forward's slots), then
    wc_unpack_host of what it returned: offsets, lengths and bytes of both."""
    packed, poff, pbytes = ctx.pack_host(B.buf if buf is None else buf,
                                         np.asarray(B.pay_off if off is None else off, np.uint64), B.units, B.n, V)
    _, doff, end = B.dense(V)
    assert poff.tolist() == doff + [end] and pbytes.tolist() == [len(p) for p in B.packed[V]]
    assert packed.size == end
    for i, want in enumerate(B.packed[V]):
        assert packed[doff[i]:doff[i] + len(want)].tobytes() == want, (B.what[i], V)
    check_unpack_host(ctx, wc, B, V, packed, poff[:B.n])


def check_unpack_host(ctx, wc, B, V, packed, poff):
    pay, o, kept = ctx.unpack_host(packed, np.asarray(poff, np.uint64), B.units, B.n)
    want_off = [4]
    for q in B.quant[V]:
        want_off.append(want_off[-1] + len(q) + 4)  # 24 + 8 kept per unit, as wc_forward_host
    want_off[-1] -= 4
    assert o.tolist() == want_off and kept.tolist() == [(len(q) - 20) // 8 for q in B.quant[V]]
    for i, want in enumerate(B.quant[V]):
        assert wc.capi.unit_payload(pay, o, kept, i) == want, (B.what[i], V)


# ------------------------------------------------------------------ the fuzz --
@pytest.mark.parametrize("V", VS)
def test_fuzz_pack_unpack_and_pack_again(ctx, F, V):
    out, poff, pbytes, _ = run_pack(ctx, F, V)
    check_packed(F, V, out, poff, pbytes)
    pay, off, kept = run_unpack(ctx, F, out, poff, F.slots[V][1])
    check_unpacked(F, F.quant[V], pay, off, kept)
    if V == 4:
        check_unpacked(F, F.pays, pay, off, kept)
    again, poff2, pbytes2, _ = run_pack(ctx, F, V, d_pay=pay, d_off=off)
    check_packed(F, V, again, poff2, pbytes2)
    buf, doff, end = F.dense(V)
    pay, off, kept = run_unpack(ctx, F, dev(buf), u64(doff), end)
    check_unpacked(F, F.quant[V], pay, off, kept)


@pytest.mark.parametrize("V", VS)
def test_fuzz_host_forms(ctx, wc, F, V):
    check_host_forms(ctx, wc, F, V)


# ---------------------------------------------------------------- many units --
@pytest.mark.parametrize("n", MANY)
def test_many_units(ctx, wc, M, n):
    """k_dense_offsets<false> (wc_pack_host) and <true> (wc_unpack_host) over n
    units: a wave is 64 units, a pass 1024.  And the device pair, whose
    descriptors and tile list have n entries."""
    B = M.head(wc, n)
    check_host_forms(ctx, wc, B, 3)
    out, poff, pbytes, _ = run_pack(ctx, B, 3)
    check_packed(B, 3, out, poff, pbytes)
    pay, off, kept = run_unpack(ctx, B, out, poff, B.slots[3][1])
    check_unpacked(B, B.quant[3], pay, off, kept)


# ----------------------------------------------------------------- the limit --
def test_limit_unit_all_pairs(ctx, wc, LIMIT):
    B = LIMIT[0]
    assert B.dims == [PR.LIMIT_DIMS] and len(B.pays[0]) == 20 + 8 * 2 ** 21
    out, poff, pbytes, _ = run_pack(ctx, B, 3)
    check_packed(B, 3, out, poff, pbytes)
    pay, off, kept = run_unpack(ctx, B, out, poff, B.slots[3][1])
    check_unpacked(B, B.quant[3], pay, off, kept)
    check_host_forms(ctx, wc, B, 3)


def test_limit_unit_few_pairs(ctx, wc, LIMIT):
    """100 pairs on the descriptors of the 2^21-cell unit: one of its 1024
    workgroups has work, and the sentinels show that the others wrote nothing."""
    big, B = LIMIT
    run_pack(ctx, big, 3)  # the descriptors of these dimensions are the cached ones
    out, poff, pbytes, _ = run_pack(ctx, B, 3)
    check_packed(B, 3, out, poff, pbytes)
    pay, off, kept = run_unpack(ctx, B, out, poff, B.slots[3][1])
    check_unpacked(B, B.quant[3], pay, off, kept)
    check_host_forms(ctx, wc, B, 3)


# ------------------------------------------------------------------- layouts --
def scattered(rng, items, first, step, gaps):
    """`items` in a random order from `first` on, each start at first (mod step)
    after a gap of 0..gaps-1 steps; unit 0 never comes first.  -> (buffer, offsets, end)."""
    order = rng.permutation(len(items)).tolist()
    if order[0] == 0:
        order[0], order[len(order) // 2] = order[len(order) // 2], order[0]
    off, cur, end = [0] * len(items), first, 0
    for j in order:
        off[j] = cur
        end = cur + len(items[j])
        cur = (end - first % step + step - 1) // step * step + first % step + step * int(rng.integers(0, gaps))
    return Batch.layout(items, off, end, margin=0), off, end


@pytest.mark.parametrize("first", [8, 4100])
def test_pack_from_scattered_source_offsets(ctx, wc, F0, first):
    """d_offsets in another order, with gaps, at 0 and at 4 (mod 8); the lowest
    offset is a middle unit's and is 0 (mod 8) or 4 (mod 8) and far from 0."""
    B, V = F0, 3
    buf, off, end = scattered(np.random.default_rng(9600 + first), B.pays, first, 4, 8)
    assert {o % 8 for o in off} == {0, 4} and min(off) == first and off[0] != first and sorted(off) != off
    d_pay = dev(buf)
    out, poff, pbytes, _ = run_pack(ctx, B, V, d_pay=d_pay, d_off=u64(off))
    check_packed(B, V, out, poff, pbytes)
    assert host(d_pay).tobytes() == buf.tobytes()
    check_host_forms(ctx, wc, B, V, buf=buf, off=off)


@pytest.mark.parametrize("first", [12, 4100])
def test_unpack_from_scattered_packed_offsets(ctx, wc, F1, first):
    """Packed offsets in another order with gaps of multiples of 8; the capacity
    is the end of the highest unit."""
    B, V = F1, 2
    buf, off, end = scattered(np.random.default_rng(9700 + first), B.packed[V], first, 8, 5)
    assert off != sorted(off) and all(o % 8 == 4 for o in off) and buf.size == end
    spans = sorted((o, o + len(p)) for o, p in zip(off, B.packed[V]))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and any(b[0] - a[1] >= 8 for a, b in zip(spans, spans[1:]))
    d_pk = dev(buf)
    pay, o, kept = run_unpack(ctx, B, d_pk, u64(off), buf.size)
    check_unpacked(B, B.quant[V], pay, o, kept)
    assert host(d_pk).tobytes() == buf.tobytes()
    check_unpack_host(ctx, wc, B, V, buf, off)


# ------------------------------------------------------- the descriptor cache --
def buffers(B, V):
    cap = B.slots[V][1]
    return types.SimpleNamespace(cap=cap, src=dev(B.buf), soff=u64(B.pay_off), out=filled(cap + 64),
                                 poff=filled(8 * (B.n + 1)), pbytes=filled(8 * B.n), pay=filled(B.pay_cap + 64),
                                 off=filled(8 * (B.n + 1)), kept=filled(4 * B.n))


def enqueue_pair(ctx, B, V, b):
    ctx.pack(b.src.data_ptr(), b.soff.data_ptr(), B.units, B.n, V, b.out.data_ptr(), b.cap, b.poff.data_ptr(),
             b.pbytes.data_ptr())
    ctx.unpack(b.out.data_ptr(), b.poff.data_ptr(), b.cap, B.units, B.n, b.pay.data_ptr(), B.pay_cap, b.off.data_ptr(),
               b.kept.data_ptr())


def test_descriptor_cache_over_changing_batches_unsynced(wc, F0, F1, M):
    """A fresh context; batch A at V = 3, batch B (as many units, other dimensions)
    at V = 2, batch C (another count) at V = 4 and batch A at V = 3 again, each
    pack + unpack into buffers of its own, with no wc_synchronize until the end."""
    C = Batch(wc, list(zip(M.what[:65], M.pays[:65])))
    assert F0.n == F1.n != C.n and F0.dims != F1.dims
    steps = [(F0, 3), (F1, 2), (C, 4), (F0, 3)]
    bufs = [buffers(B, V) for B, V in steps]  # every allocation and upload before the first call
    ctx = wc.capi.Context(0)
    try:
        for (B, V), b in zip(steps, bufs):
            enqueue_pair(ctx, B, V, b)
        ctx.synchronize()
        for (B, V), b in zip(steps, bufs):
            check_packed(B, V, b.out, b.poff, b.pbytes)
            check_unpacked(B, B.quant[V], b.pay, b.off, b.kept)
    finally:
        ctx.close()


# -------------------------------------------------------------- the pipeline --
class Pipe(Batch):
    """The field units of pack_rule.NATURAL and a unit without cells, as cells for
    wc_forward_levels at keep 0.99; the payloads are levels_ref's."""

    def __init__(self, wc, V):
        spec = [(what, d, L, kind) for what, d, L, kind, _ in PR.NATURAL] + [("empty", (0, 4, 4), 1, 0)]
        boxes = [field(kind, W, H, D, 9800 + i) if W * H * D else np.zeros((D, H, W), np.float32)
                 for i, (_, (W, H, D), _, kind) in enumerate(spec)]
        super().__init__(wc, [(s[0], LR.payload(b, s[2], keep=KEEP)[0], True) for s, b in zip(spec, boxes)], vs=(V,))
        assert self.levels == [s[2] for s in spec]
        self.cells = np.zeros(self.extent + 8, np.float32)
        for u, b in zip(self.units, boxes):
            self.cells[u.cell_offset:u.cell_offset + b.size] = b.ravel()
        self.decoded = [LR.decode(q)[0] for q in self.quant[V]]
        self.V = V

    def device(self):
        import torch
        b = buffers(self, self.V)
        b.cells = dev(self.cells)
        b.fpay, b.foff, b.fkept = filled(self.pay_cap + 64), filled(8 * (self.n + 1)), filled(4 * self.n)
        b.back = torch.full((self.extent + 8,), -77.0, dtype=torch.float32, device=b.cells.device)
        torch.cuda.synchronize()
        return b

    def enqueue(self, wc, ctx, b):
        ctx.forward_levels(b.cells.data_ptr(), wc.capi.WC_F32, self.units, self.n, self.levels, KEEP, None,
                           b.fpay.data_ptr(), self.pay_cap, b.foff.data_ptr(), b.fkept.data_ptr())
        ctx.pack(b.fpay.data_ptr(), b.foff.data_ptr(), self.units, self.n, self.V, b.out.data_ptr(), b.cap,
                 b.poff.data_ptr(), b.pbytes.data_ptr())
        ctx.unpack(b.out.data_ptr(), b.poff.data_ptr(), b.cap, self.units, self.n, b.pay.data_ptr(), self.pay_cap,
                   b.off.data_ptr(), b.kept.data_ptr())
        ctx.inverse_levels(b.pay.data_ptr(), b.off.data_ptr(), self.units, self.n, self.levels, b.back.data_ptr())

    def check(self, out, poff, pbytes, pay, off, kept, back):
        check_packed(self, self.V, out, poff, pbytes)
        check_unpacked(self, self.quant[self.V], pay, off, kept)
        got = back.cpu().numpy().view(np.float32)
        for i, (u, want) in enumerate(zip(self.units, self.decoded)):
            assert got[u.cell_offset:u.cell_offset + want.size].tobytes() == want.tobytes(), self.what[i]


@pytest.fixture(scope="module")
def P(wc):
    return Pipe(wc, 3)


def test_pipeline_without_a_host_sync(wc, P):
    """wc_forward_levels writes headers, pairs and d_offsets; wc_pack reads them;
    wc_unpack and wc_inverse_levels follow.  A fresh context, one wc_synchronize."""
    assert max(P.levels) == 3 and min(len(p) for p in P.pays) == 20
    b = P.device()
    ctx = wc.capi.Context(0)
    try:
        P.enqueue(wc, ctx, b)
        ctx.synchronize()
        P.check(b.out, b.poff, b.pbytes, b.pay, b.off, b.kept, b.back)
    finally:
        ctx.close()


def test_pipeline_on_a_caller_stream(wc, P):
    """The same chain on a torch stream s after wc_set_stream(s), behind a delay
    and the producer of the cells; clones of the outputs and their overwrite
    follow, all without a host sync.  After s.synchronize() the clones hold the
    restatement's bytes."""
    import torch
    b = P.device()
    outs = (b.out, b.poff, b.pbytes, b.pay, b.off, b.kept, b.back)
    ctx = wc.capi.Context(0)
    s = torch.cuda.Stream()
    try:
        P.enqueue(wc, ctx, b)  # once with plain syncs: plans and descriptors are uploaded, nothing afterwards allocates
        ctx.synchronize()
        with torch.cuda.stream(s):
            spare = [t.clone() for t in outs]
        s.synchronize()
        del spare
        for t in outs[:-1] + (b.fpay, b.foff, b.fkept):
            t.fill_(SENT)
        b.back.fill_(-77.0)
        real = b.cells.clone()
        b.cells.zero_()
        torch.cuda.synchronize()
        ctx.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            torch.cuda._sleep(100_000_000)
            b.cells.copy_(real)
            P.enqueue(wc, ctx, b)
            c = [t.clone() for t in outs]
            for t in outs:
                t.fill_(0)
            b.cells.fill_(7.0)
            busy = not s.query()
        assert busy, "the stream was idle right after the last enqueue: a call blocked, so this test had no power"
        s.synchronize()
        P.check(*c)
        ctx.synchronize()
    finally:
        ctx.set_stream(None)
        ctx.close()
