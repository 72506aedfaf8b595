"""GPU: the asynchronous contract of the device-pointer entry points
(include/wavelet_amd.h, Conventions and wc_set_stream): every call is
asynchronous on the context's stream, wc_set_stream moves the context onto a
caller's stream, and the small host arrays (tol, levels, reduce) are consumed
before the call returns.  The other GPU tests bracket every device call with a
host synchronise, so none of this is visible to them.

  1. producer -> library -> consumer on a torch stream, no host sync in between;
  2. switching streams: the drain, the next call on the context's own stream,
     the kernel error word across a switch, two contexts on two streams;
  3. the pipelined inverse (WC_OPT_INV_GROUPS) joins its second stream back onto
     the caller's stream, not only onto wc_synchronize;
  4. unsynced chains of calls over different batches on one fresh context (scratch
     growth, plan cache hits and evictions, stale row-index granules, the pinned
     block shared by the tolerance / levels / coarse calls);
  5. wc_profile_enable / wc_profile_read.

Every expectation is the CPU oracle's (or the modes' CPU restatements
tol_rule.py, levels_ref.py, coarse_ref.py), computed once per batch.  Every test
owns its context, so the session's context never sits on a foreign stream.

The stream tests hold a stream busy with torch.cuda._sleep, calibrated once per
module to about DELAY_MS.  The length is not a tolerance: each test that relies
on the delay asserts that the stream was still busy after the last enqueue and
fails, saying it had no power, if it was not.
"""
import ctypes
import math

import numpy as np
import pytest

import coarse_ref
import levels_ref
import numpy_ref
from test_gpu_fuzz import same_cells
from tol_rule import same_bits, tol_rule
from wavelet_compression_amd.capi import (WC_ERR_FORMAT, WC_ERR_INVALID, WC_OK, WC_OPT_INV_GROUPS,
                                          WC_OPT_TOL_SOLO_TILES, WaveletError)

pytestmark = pytest.mark.gpu

KEEP = float(np.float32(0.999))
DELAY_MS = 50.0
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]

ROWS = [(64, 64, 64), (32, 32, 32), (16, 32, 64), (48, 32, 16), (8, 4, 8), (2, 2, 8)]  # row-indexed, fast, sparse
GENERIC = [(3, 5, 7), (6, 10, 14), (33, 17, 9), (5, 1, 9)]                            # generic path, dense decode
EMPTY = (4, 4, 0)
BATCHES = {
    # name: (dims, units at an odd cell offset, field seed)
    "base": (ROWS + GENERIC + [EMPTY], (2, 7), 71),
    "other": (GENERIC + [(16, 32, 64), (32, 32, 32), EMPTY, (48, 32, 16)], (1, 4), 72),
    "groups": ([(64, 64, 64)] * 8 + [(3, 5, 7), (33, 17, 9)], (), 73),
    "groups_rix": ([(64, 64, 64)] * 8, (), 75),  # nothing follows the last group's row index on the caller's stream
    "header": ([(16, 16, 16), (32, 32, 32)], (), 74),
    # ascending: about 400, 34 k, 290 k and 0.9 M cells
    "chain0": ([(8, 4, 8), (3, 5, 7), EMPTY, (2, 2, 8)], (1,), 80),
    "chain1": ([(32, 32, 32), (6, 10, 14), (5, 1, 9)], (2,), 81),
    "chain2": ([(64, 64, 64), (48, 32, 16), (33, 17, 9), (8, 4, 8)], (1,), 82),
    "chain3": ([(64, 64, 64)] * 3 + [(16, 32, 64), (3, 5, 7), (16, 32, 64), (32, 32, 32), (48, 32, 16), (6, 10, 14)],
               (3, 8), 83),
    # every dimension divisible by 8: levels 1..3 and the tolerance mode take them all
    "modes": ([(16, 16, 16), (32, 32, 32), (16, 32, 64), (48, 32, 16), (8, 8, 8), (64, 64, 64), (8, 16, 24)], (), 84),
}
for _k in range(20):  # plan eviction: more distinct batches than the plan cache holds
    BATCHES["tiny%d" % _k] = ([(2, 2, 8), (3, 5, 7), (_k + 1, 2, 4)], (1,), 90 + _k)


class Batch:
    """The units and cells of one batch of smooth oracle fields, and what the
    oracle computes from them (once, on demand)."""

    def __init__(self, wc, O, dims, odd, seed, dtype):
        self.wc, self.O, self.dims, self.dtype = wc, O, list(dims), dtype
        self.offs, cur = [], 0
        for i, (W, H, D) in enumerate(dims):
            cur = (cur + 3) // 4 * 4 + (1 if i in odd else 0)
            self.offs.append(cur)
            cur += W * H * D
        self.units, self.n, self.extent = wc.capi.make_units(dims, offsets=self.offs)
        self.code = wc.capi.WC_F64 if dtype == np.float64 else wc.capi.WC_F32
        self.cap = wc.capi.payload_bound(self.units, self.n)
        self.rb = wc.capi.rowindex_bytes(self.units, self.n)
        self.host = np.zeros(max(self.extent, 1), dtype)
        self.b32 = []
        for i, (W, H, D) in enumerate(dims):
            if W * H * D == 0:
                self.b32.append(np.zeros((D, H, W), np.float32))
                continue
            b64 = O.synth_box_f64(O.unit_seed(seed, 0, i, 0), (3 * i, 5 * i, 7 * i), W, H, D)
            b = O.narrow(b64) if dtype == np.float64 else b64.astype(np.float32)
            self.host[self.offs[i]:self.offs[i] + b.size] = (b64 if dtype == np.float64 else b).ravel()
            self.b32.append(b)
        self.slots = [4]  # wc_forward's fixed slots
        for W, H, D in dims:
            self.slots.append(self.slots[-1] + 24 + 8 * W * H * D)
        self._six = self._modes = None

    def six(self):
        """Per unit: payload bytes, kept, decompress(), wavelet_decompose(), its
        inverse, both RMSEs, the row index of the row-indexable units."""
        if self._six is None:
            O, e = self.O, []
            for b, (W, H, D) in zip(self.b32, self.dims):
                if b.size == 0:
                    z = np.zeros(0, np.float32)
                    e.append(dict(pay=np.array([W, H, D, 0, 0], "<i4").tobytes(), kept=0, back=z, flat=z, full=z))
                    continue
                pay, kept = O.compress_payload(b, KEEP)
                back = O.decompress_payload(pay)
                flat = O.wavelet_decompose(b)
                full = O.inverse_wavelet_decompose(flat, W, H, D)
                u = dict(pay=pay, kept=kept, back=back.ravel(), flat=flat, full=full.ravel(),
                         r_back=O.rmse(b, back), r_full=O.rmse(b, full))
                if W % 2 == 0 and H % 2 == 0 and D % 8 == 0:
                    u["rows"] = numpy_ref.row_index(pay, W, H, D)
                e.append(u)
            self._six = e
        return self._six


_BATCHES = {}


def batch(wc, O, name, dtype):
    key = (name, np.dtype(dtype).name)
    if key not in _BATCHES:
        dims, odd, seed = BATCHES[name]
        _BATCHES[key] = Batch(wc, O, dims, odd, seed, dtype)
    return _BATCHES[key]


SIX = ("pay", "po", "kept", "rows", "out1", "r1", "out2", "flat", "out3", "r2")


class Outs:
    """Device outputs of the six calls of enqueue_six, pre-filled with values no
    call writes (allocated and filled on torch's current stream)."""

    def __init__(self, torch, B, tensors=None):
        self.torch = torch
        if tensors is not None:
            self.__dict__.update(tensors)
            return
        dev, n, ext = torch.device("cuda", 0), B.n, max(B.extent, 1)
        self.pay = torch.zeros(B.cap, dtype=torch.uint8, device=dev)
        self.po = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        self.kept = torch.zeros(n, dtype=torch.int32, device=dev)
        self.rows = torch.zeros(max(B.rb // 8, 1), dtype=torch.int64, device=dev)
        for name in ("out1", "out2", "flat", "out3"):
            setattr(self, name, torch.full((ext,), float("nan"), dtype=torch.float32, device=dev))
        for name in ("r1", "r2"):
            setattr(self, name, torch.full((n,), float("nan"), dtype=torch.float64, device=dev))

    def clones(self):
        return Outs(self.torch, None, {k: getattr(self, k).clone() for k in SIX})

    def scrub(self):
        """What a caller that reuses its buffers does next, on the current stream."""
        for k in ("pay", "po", "kept", "rows"):
            getattr(self, k).zero_()
        for k in ("out1", "out2", "flat", "out3", "r1", "r2"):
            getattr(self, k).fill_(float("nan"))

    def host(self):
        return {k: getattr(self, k).cpu().numpy() for k in SIX}


def enqueue_six(ctx, B, cells, o):
    """wc_forward_rows, wc_inverse_rows with the fused RMSE, wc_inverse from the
    payloads alone, wc_decompose, wc_inverse_flat, wc_rmse: no host sync.  The
    binding raises unless a call returns WC_OK."""
    u, n = B.units, B.n
    ctx.forward_rows(cells.data_ptr(), B.code, u, n, KEEP, o.pay.data_ptr(), B.cap, o.po.data_ptr(),
                     o.kept.data_ptr(), o.rows.data_ptr(), B.rb)
    ctx.inverse_rows(o.pay.data_ptr(), o.po.data_ptr(), u, n, o.rows.data_ptr(), o.out1.data_ptr(), cells.data_ptr(),
                     B.code, o.r1.data_ptr())
    ctx.inverse(o.pay.data_ptr(), o.po.data_ptr(), u, n, o.out2.data_ptr())
    ctx.decompose(cells.data_ptr(), B.code, u, n, o.flat.data_ptr())
    ctx.inverse_flat(o.flat.data_ptr(), u, n, o.out3.data_ptr())
    ctx.rmse(cells.data_ptr(), B.code, o.out3.data_ptr(), u, n, o.r2.data_ptr())


def check_rmse(got, ref, cells, what):
    # the fuzz test's bound (test_gpu_fuzz.py: the same n exact double terms in another order)
    tol = max(1e-12, (cells + 4) * 2.0 ** -53)
    assert abs(got - ref) <= tol * abs(ref), (what, got, ref)


def check_forward(B, pay, po, kept, what, want=None):
    """Payload bytes, slot offsets and kept counts, exactly."""
    want = want or [(u["pay"], u["kept"]) for u in B.six()]
    n = B.n
    assert [int(x) for x in kept] == [k for _, k in want], (what, "kept")
    assert [int(x) for x in po] == B.slots[:n] + [B.slots[n - 1] + 20 + 8 * want[n - 1][1]], (what, "offsets")
    for i, (p, k) in enumerate(want):
        assert pay[B.slots[i]:B.slots[i] + 20 + 8 * k].tobytes() == p, (what, i, B.dims[i], "payload")


def check_six(B, h, what):
    check_forward(B, h["pay"], h["po"], h["kept"], what)
    rows = h["rows"].view(np.uint32).reshape(-1, 2)
    ent = 0
    for i, (u, (W, H, D)) in enumerate(zip(B.six(), B.dims)):
        cells, o = W * H * D, B.offs[i]
        if not cells:
            continue
        w = (what, i, B.dims[i])
        if "rows" in u:
            assert np.array_equal(rows[ent:ent + W * H + 1], u["rows"]), (w, "row index")
        ent += W * H + 1
        assert same_cells(h["out1"][o:o + cells], u["back"]), (w, "inverse_rows")
        assert same_cells(h["out2"][o:o + cells], u["back"]), (w, "inverse")
        assert same_cells(h["flat"][o:o + cells], u["flat"]), (w, "decompose")
        assert same_cells(h["out3"][o:o + cells], u["full"]), (w, "inverse_flat")
        check_rmse(h["r1"][i], u["r_back"], cells, (w, "fused rmse"))
        check_rmse(h["r2"][i], u["r_full"], cells, (w, "rmse"))


@pytest.fixture(scope="module")
def delay_cycles():
    """torch.cuda._sleep cycles for about DELAY_MS, from one timed probe."""
    import torch
    probe = 2_000_000
    torch.cuda._sleep(probe)  # the first launch loads the kernel
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(probe)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b)
    assert ms > 0.0, ms
    return max(probe, int(probe * DELAY_MS / ms))


NO_POWER = ("the stream was idle right after the last enqueue: a call blocked or the delay was too short, "
            "so this test had no power")


def device_cells(torch, B):
    return torch.from_numpy(B.host).to(torch.device("cuda", 0))


def warm(torch, ctx, B, cells, o, s):
    """The same sequence once with plain syncs, so that nothing afterwards builds
    a plan, grows a buffer or allocates a clone's memory."""
    torch.cuda.synchronize()
    enqueue_six(ctx, B, cells, o)
    ctx.synchronize()
    with torch.cuda.stream(s):
        c = o.clones()
    s.synchronize()
    del c
    o.scrub()
    torch.cuda.synchronize()


# ---- 1. producer and consumer ordering on a caller's stream --------------------------------


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_caller_stream_orders_producer_and_consumer(wc, oracle, delay_cycles, dtype):
    """On a torch stream s, after wc_set_stream(s): a delay, then the producer
    (cells.copy_), the six calls, a clone of every output and the overwrite of
    the originals, all enqueued without a host sync.  After s.synchronize()
    alone the clones hold the oracle's results: the calls ran after the producer
    (the cells held zeros before it, which would give kept == 0) and before the
    overwrite."""
    import torch
    B = batch(wc, oracle, "base", dtype)
    ctx = wc.capi.Context(0)
    s = torch.cuda.Stream()
    try:
        real = device_cells(torch, B)
        cells = real.clone()
        o = Outs(torch, B)
        warm(torch, ctx, B, cells, o, s)
        cells.zero_()
        torch.cuda.synchronize()
        ctx.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            torch.cuda._sleep(delay_cycles)
            cells.copy_(real)
            enqueue_six(ctx, B, cells, o)  # (a): raises unless every call returns WC_OK
            c = o.clones()
            o.scrub()
            cells.fill_(float("nan"))
            busy = not s.query()
        assert busy, NO_POWER  # (b)
        s.synchronize()  # (c): the torch sync only, no wc_synchronize before the comparison
        check_six(B, c.host(), "caller stream")
        ctx.synchronize()  # (d)
    finally:
        ctx.set_stream(None)
        ctx.close()


# ---- 2. switching streams ------------------------------------------------------------------


def test_set_stream_none_drains_the_callers_stream(wc, oracle, delay_cycles):
    """wc_set_stream(NULL) returns only after the caller's stream has drained; the
    next call runs on the context's own stream and is right after wc_synchronize.
    torch's default stream has handle 0, which selects the context's own stream
    (Streams)."""
    import torch
    assert torch.cuda.default_stream().cuda_stream == 0
    B = batch(wc, oracle, "base", np.float64)
    ctx = wc.capi.Context(0)
    s = torch.cuda.Stream()
    try:
        cells = device_cells(torch, B)
        o = Outs(torch, B)
        warm(torch, ctx, B, cells, o, s)
        ctx.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            torch.cuda._sleep(delay_cycles)
            ctx.forward(cells.data_ptr(), B.code, B.units, B.n, KEEP, o.pay.data_ptr(), B.cap, o.po.data_ptr(),
                        o.kept.data_ptr())
            busy = not s.query()
        assert busy, NO_POWER
        ctx.set_stream(None)
        assert s.query(), "wc_set_stream returned with work still queued on the previous stream"
        ctx.inverse(o.pay.data_ptr(), o.po.data_ptr(), B.units, B.n, o.out2.data_ptr())
        ctx.synchronize()
        h = o.host()
        check_forward(B, h["pay"], h["po"], h["kept"], "before the switch")
        for i, u in enumerate(B.six()):
            assert same_cells(h["out2"][B.offs[i]:B.offs[i] + u["back"].size], u["back"]), (i, B.dims[i])
    finally:
        ctx.set_stream(None)
        ctx.close()


def test_error_word_survives_a_stream_switch(wc, oracle):
    """A header that disagrees with its unit (nothing past it is read), decoded on
    a caller's stream: after wc_set_stream(NULL) the next wc_synchronize raises
    WC_ERR_FORMAT exactly once, the one after it is clean, and a good decode
    that follows is exact."""
    import torch
    B = batch(wc, oracle, "header", np.float64)
    ctx = wc.capi.Context(0)
    s = torch.cuda.Stream()
    try:
        cells = device_cells(torch, B)
        o = Outs(torch, B)
        torch.cuda.synchronize()
        ctx.forward_rows(cells.data_ptr(), B.code, B.units, B.n, KEEP, o.pay.data_ptr(), B.cap, o.po.data_ptr(),
                         o.kept.data_ptr(), o.rows.data_ptr(), B.rb)
        ctx.synchronize()
        p1 = B.slots[1]
        o.pay[p1:p1 + 4] = torch.tensor(np.array([33], "<i4").view(np.uint8), device=o.pay.device)  # W 32 -> 33
        torch.cuda.synchronize()
        ctx.set_stream(s.cuda_stream)
        ctx.inverse_rows(o.pay.data_ptr(), o.po.data_ptr(), B.units, B.n, o.rows.data_ptr(), o.out1.data_ptr())
        ctx.set_stream(None)
        with pytest.raises(WaveletError) as e:
            ctx.synchronize()
        assert e.value.code == WC_ERR_FORMAT
        ctx.synchronize()  # reported once
        o.pay[p1:p1 + 4] = torch.tensor(np.array([32], "<i4").view(np.uint8), device=o.pay.device)
        o.out1.fill_(float("nan"))
        torch.cuda.synchronize()
        ctx.inverse_rows(o.pay.data_ptr(), o.po.data_ptr(), B.units, B.n, o.rows.data_ptr(), o.out1.data_ptr())
        ctx.synchronize()
        out = o.out1.cpu().numpy()
        for i, u in enumerate(B.six()):
            assert same_cells(out[B.offs[i]:B.offs[i] + u["back"].size], u["back"]), (i, B.dims[i])
    finally:
        ctx.set_stream(None)
        ctx.close()


def test_two_contexts_on_two_streams(wc, oracle, delay_cycles):
    """Two contexts, each on its own torch stream behind its own delay, on
    different batches: both match the oracle after their stream's sync alone."""
    import torch
    Bs = [batch(wc, oracle, "base", np.float64), batch(wc, oracle, "other", np.float32)]
    ctxs = [wc.capi.Context(0), wc.capi.Context(0)]
    ss = [torch.cuda.Stream(), torch.cuda.Stream()]
    try:
        cells = [device_cells(torch, B) for B in Bs]
        outs = [Outs(torch, B) for B in Bs]
        for ctx, B, c, o, s in zip(ctxs, Bs, cells, outs, ss):
            warm(torch, ctx, B, c, o, s)
            ctx.set_stream(s.cuda_stream)
        for s in ss:
            with torch.cuda.stream(s):
                torch.cuda._sleep(delay_cycles)
        clones = []
        for ctx, B, c, o, s in zip(ctxs, Bs, cells, outs, ss):
            with torch.cuda.stream(s):
                enqueue_six(ctx, B, c, o)
                clones.append(o.clones())
                o.scrub()
        busy = [not s.query() for s in ss]
        assert all(busy), (NO_POWER, busy)
        for s, B, c in zip(ss, Bs, clones):
            s.synchronize()
            check_six(B, c.host(), "two contexts")
        for ctx in ctxs:
            ctx.synchronize()
    finally:
        for ctx in ctxs:
            ctx.set_stream(None)
            ctx.close()


# ---- 3. the aux stream joins the caller's stream -------------------------------------------


@pytest.mark.parametrize("name", ["groups", "groups_rix"])
@pytest.mark.parametrize("groups", [2, 3])
def test_pipelined_inverse_joins_the_callers_stream(wc, oracle, delay_cycles, groups, name):
    """WC_OPT_INV_GROUPS > 1 reconstructs group g on a second stream of the
    context.  A consumer ordered on the caller's stream alone (out.clone() on s,
    then s.synchronize(), never wc_synchronize, which drains the second stream
    itself) sees every cell: the clone equals the oracle and the pre-fill NaN
    survives nowhere inside a unit; wc_inverse_rmse likewise.  A missing join
    shows only as a race between the clone and the last group's reconstruction,
    so this test is likely, not certain, to catch one.  Two batches: eight 64^3
    units with two dense-decode units, whose decode and inverse run on the
    caller's stream after the last group's row index and give the second stream
    a head start; and the eight 64^3 units alone, where the clone follows the
    last row index directly.  (Against a build with the join taken out, the
    second batch failed at both group counts and the first one passed.)  With
    profiling on the call takes the unpiped path; the cells are the same."""
    import torch
    B = batch(wc, oracle, name, np.float64)
    u, n = B.units, B.n
    ctx = wc.capi.Context(0)
    s = torch.cuda.Stream()
    before = ctx.get_option(WC_OPT_INV_GROUPS)
    try:
        ctx.set_option(WC_OPT_INV_GROUPS, groups)
        cells = device_cells(torch, B)
        o = Outs(torch, B)
        torch.cuda.synchronize()
        ctx.forward(cells.data_ptr(), B.code, u, n, KEEP, o.pay.data_ptr(), B.cap, o.po.data_ptr(), o.kept.data_ptr())
        # warm: the second stream and its events, the clones' memory
        ctx.inverse(o.pay.data_ptr(), o.po.data_ptr(), u, n, o.out1.data_ptr())
        ctx.inverse_rmse(o.pay.data_ptr(), o.po.data_ptr(), u, n, cells.data_ptr(), B.code, o.out2.data_ptr(),
                         o.r1.data_ptr())
        ctx.synchronize()
        with torch.cuda.stream(s):
            c = [o.out1.clone(), o.out2.clone(), o.r1.clone()]
        s.synchronize()
        del c
        for t in (o.out1, o.out2, o.r1):
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        ctx.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            torch.cuda._sleep(delay_cycles)
            ctx.inverse(o.pay.data_ptr(), o.po.data_ptr(), u, n, o.out1.data_ptr())
            c1 = o.out1.clone()
            ctx.inverse_rmse(o.pay.data_ptr(), o.po.data_ptr(), u, n, cells.data_ptr(), B.code, o.out2.data_ptr(),
                             o.r1.data_ptr())
            c2, cr = o.out2.clone(), o.r1.clone()
            busy = not s.query()
        assert busy, NO_POWER
        s.synchronize()  # the torch sync only
        h1, h2, hr = c1.cpu().numpy(), c2.cpu().numpy(), cr.cpu().numpy()
        for i, e in enumerate(B.six()):
            a, cnt = B.offs[i], e["back"].size
            for tag, h in (("inverse", h1), ("inverse_rmse", h2)):
                assert not np.isnan(h[a:a + cnt]).any(), (groups, i, tag, "pre-fill survives")
                assert same_cells(h[a:a + cnt], e["back"]), (groups, i, tag)
            check_rmse(hr[i], e["r_back"], cnt, (groups, i))
        ctx.synchronize()
        ctx.profile_enable(True)
        with torch.cuda.stream(s):
            o.out1.fill_(float("nan"))
            ctx.inverse(o.pay.data_ptr(), o.po.data_ptr(), u, n, o.out1.data_ptr())
            c3 = o.out1.clone()
        s.synchronize()
        assert same_cells(c3.cpu().numpy(), h1), (groups, "profiling on")
        ctx.profile_enable(False)
        assert set(ctx.profile_read()) == {"decode", "inverse"}
    finally:
        ctx.set_stream(None)
        ctx.set_option(WC_OPT_INV_GROUPS, before)
        ctx.close()


# ---- 4. unsynced chains over different batches on one context ------------------------------


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unsynced_chain_over_growing_batches(wc, oracle, dtype):
    """A fresh context (every scratch buffer still to grow): four batches of
    ascending size, the six calls each into the batch's own outputs with no sync
    between batches, then the batches again in reverse order into fresh outputs
    (plan cache hits, no growth, row-index granules of earlier epochs in place).
    One wc_synchronize at the end; all eight result sets are the oracle's."""
    import torch
    Bs = [batch(wc, oracle, "chain%d" % k, dtype) for k in range(4)]
    assert [sum(W * H * D for W, H, D in B.dims) for B in Bs] == sorted(sum(W * H * D for W, H, D in B.dims) for B in Bs)
    ctx = wc.capi.Context(0)
    try:
        cells = [device_cells(torch, B) for B in Bs]
        up = [Outs(torch, B) for B in Bs]
        down = [Outs(torch, B) for B in Bs]
        torch.cuda.synchronize()
        for B, c, o in zip(Bs, cells, up):
            enqueue_six(ctx, B, c, o)
        for B, c, o in reversed(list(zip(Bs, cells, down))):
            enqueue_six(ctx, B, c, o)
        ctx.synchronize()
        for k, B in enumerate(Bs):
            check_six(B, up[k].host(), ("ascending", k))
            check_six(B, down[k].host(), ("descending", k))
    finally:
        ctx.close()


def test_unsynced_forwards_past_the_plan_cache(wc, oracle):
    """20 tiny distinct batches forward back to back into separate outputs (the
    plan cache holds 16: the last ones build their plans into evicted plans'
    device buffers while earlier kernels are queued), then the first four again
    (evicted by then), one sync at the end."""
    import torch
    Bs = [batch(wc, oracle, "tiny%d" % k, np.float64) for k in range(20)]
    order = Bs + Bs[:4]
    ctx = wc.capi.Context(0)
    try:
        cells = {id(B): device_cells(torch, B) for B in Bs}
        outs = [Outs(torch, B) for B in order]
        torch.cuda.synchronize()
        for B, o in zip(order, outs):
            ctx.forward(cells[id(B)].data_ptr(), B.code, B.units, B.n, KEEP, o.pay.data_ptr(), B.cap, o.po.data_ptr(),
                        o.kept.data_ptr())
        ctx.synchronize()
        for k, (B, o) in enumerate(zip(order, outs)):
            check_forward(B, o.pay.cpu().numpy(), o.po.cpu().numpy(), o.kept.cpu().numpy(), ("tiny", k))
    finally:
        ctx.close()


TOL_A = [1e-2, 0.1, 1e-3, 1.0, 0.0, math.inf, 1e-2]
TOL_B = [0.0, 1e-3, 1.0, math.inf, 0.1, 1e-2, 1.0]
LEVELS = [1, 2, 3, 1, 2, 3, 2]
REDUCE = [1, 1, 2, 0, 2, 3, 0]
HIST_Q = 0.9


def modes_expect(B):
    """The modes' CPU restatements on the "modes" batch, once: per tolerance list
    (thresh, bound, payload, kept) per unit; the multi-level payloads, their
    reconstructions and coarse decodes; the histogram and its threshold's payloads."""
    if B._modes is None:
        O = B.O
        flats = [O.wavelet_decompose(b) for b in B.b32]
        counts = [O.magnitude_hist(f) for f in flats]
        e = {}
        for name, tols in (("A", TOL_A), ("B", TOL_B)):
            e[name] = []
            for b, f, c, tol in zip(B.b32, flats, counts, tols):
                t, bound = tol_rule(c, f.size, tol)
                p = O.compress_payload_thresh(b, t)
                e[name].append((t, bound, p, int(np.frombuffer(p[16:20], "<i4")[0])))
        e["levels"] = [levels_ref.payload(b, L, keep=KEEP) for b, L in zip(B.b32, LEVELS)]
        e["cells"] = [levels_ref.decode(p)[0].ravel() for p, _ in e["levels"]]
        e["coarse"] = [coarse_ref.decode(p, r).ravel() for (p, _), r in zip(e["levels"], REDUCE)]
        e["hist"] = sum(counts)
        e["t"] = O.hist_threshold(e["hist"], HIST_Q)[0]
        e["emit_t"] = []
        for b in B.b32:
            p = O.compress_payload_thresh(b, e["t"])
            e["emit_t"].append((p, int(np.frombuffer(p[16:20], "<i4")[0])))
        e["emit_keep"] = [O.compress_payload(b, KEEP) for b in B.b32]
        B._modes = e
    return B._modes


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unsynced_modes_share_the_pinned_block(wc, oracle, dtype):
    """The calls whose host arrays travel through the context's one pinned block
    and one device block, back to back without a sync on a fresh context, each
    into its own outputs: wc_forward_tol (twice, solo and split binning),
    wc_forward_levels, wc_inverse_levels, wc_inverse_coarse, then
    wc_forward_stage with a histogram and wc_forward_emit (a threshold, then the
    keep rule).  Thresholds, bounds, payloads, cells and bins are bit-exact
    against the CPU restatements, as in the modes' own tests.

    "Consumed before the call returns": the library is called with the pointer
    of the caller's own tol / levels / reduce array, and each array is
    overwritten in place with other valid values as soon as the call returns;
    the results reflect the values at call time."""
    import torch
    B = batch(wc, oracle, "modes", dtype)
    E = modes_expect(B)
    u, n = B.units, B.n
    ctx = wc.capi.Context(0)
    L, h = ctx._L, ctx.handle
    dev = torch.device("cuda", 0)
    try:
        ctx.set_option(WC_OPT_TOL_SOLO_TILES, 4)  # 32^3, 16x32x64 and 64^3 are split, the others binned solo
        cells = device_cells(torch, B)

        def fwd_bufs():
            return (torch.zeros(B.cap, dtype=torch.uint8, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev),
                    torch.full((n,), -1, dtype=torch.int32, device=dev))

        fa, fb, fl, ft, fk = (fwd_bufs() for _ in range(5))
        th = [torch.full((n,), -7.0, dtype=torch.float32, device=dev) for _ in range(2)]
        bd = [torch.full((n,), -7.0, dtype=torch.float64, device=dev) for _ in range(2)]
        out_l = torch.full((max(B.extent, 1),), float("nan"), dtype=torch.float32, device=dev)
        cu, cext = wc.capi.coarse_units(u, n, REDUCE)
        out_c = torch.full((max(cext, 1),), float("nan"), dtype=torch.float32, device=dev)
        hist = torch.zeros(wc.capi.HIST_BINS, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        tol_a, tol_b = np.array(TOL_A, np.float64), np.array(TOL_B, np.float64)
        lv = [np.array(LEVELS, np.int32) for _ in range(3)]
        rd = np.array(REDUCE, np.int32)
        rcs = []
        for tol, (p, po, k), t, b in ((tol_a, fa, th[0], bd[0]), (tol_b, fb, th[1], bd[1])):
            rcs.append(L.wc_forward_tol(h, cells.data_ptr(), B.code, u, n, tol.ctypes.data, p.data_ptr(), B.cap,
                                        po.data_ptr(), k.data_ptr(), t.data_ptr(), b.data_ptr()))
            tol[:] = 7.0 if tol is tol_a else 0.0
        rcs.append(L.wc_forward_levels(h, cells.data_ptr(), B.code, u, n, lv[0].ctypes.data, KEEP, None,
                                       fl[0].data_ptr(), B.cap, fl[1].data_ptr(), fl[2].data_ptr()))
        lv[0][:] = 1
        rcs.append(L.wc_inverse_levels(h, fl[0].data_ptr(), fl[1].data_ptr(), u, n, lv[1].ctypes.data, out_l.data_ptr()))
        lv[1][:] = 1
        rcs.append(L.wc_inverse_coarse(h, fl[0].data_ptr(), fl[1].data_ptr(), u, n, lv[2].ctypes.data, rd.ctypes.data,
                                       cu, out_c.data_ptr()))
        lv[2][:] = 1
        rd[:] = 0
        ctx.forward_stage(cells.data_ptr(), B.code, u, n, hist.data_ptr())
        ctx.forward_emit(u, n, 0.0, E["t"], ft[0].data_ptr(), B.cap, ft[1].data_ptr(), ft[2].data_ptr())
        ctx.forward_emit(u, n, KEEP, None, fk[0].data_ptr(), B.cap, fk[1].data_ptr(), fk[2].data_ptr())
        assert rcs == [WC_OK] * 5, (rcs, L.wc_last_error(h))
        ctx.synchronize()

        def host(f):
            return f[0].cpu().numpy(), f[1].cpu().numpy(), f[2].cpu().numpy()

        for name, f, t, b, tols in (("A", fa, th[0], bd[0], TOL_A), ("B", fb, th[1], bd[1], TOL_B)):
            check_forward(B, *host(f), ("forward_tol", name), [(p, k) for _, _, p, k in E[name]])
            t, b = t.cpu().numpy(), b.cpu().numpy()
            for i, (wt, wb, _, _) in enumerate(E[name]):
                assert same_bits(float(t[i]), wt, np.float32), (name, i, float(t[i]), wt, tols[i])
                assert same_bits(float(b[i]), wb), (name, i, float(b[i]), wb, tols[i])
        check_forward(B, *host(fl), "forward_levels", E["levels"])
        got_l, got_c = out_l.cpu().numpy(), out_c.cpu().numpy()
        for i, (W, H, D) in enumerate(B.dims):
            assert same_cells(got_l[B.offs[i]:B.offs[i] + W * H * D], E["cells"][i]), (i, "inverse_levels", LEVELS[i])
            a = cu[i].cell_offset
            assert same_cells(got_c[a:a + E["coarse"][i].size], E["coarse"][i]), (i, "inverse_coarse", REDUCE[i])
        assert np.array_equal(hist.cpu().numpy().view(np.uint64), E["hist"])
        check_forward(B, *host(ft), "forward_emit at a threshold", E["emit_t"])
        check_forward(B, *host(fk), "forward_emit with keep", E["emit_keep"])
    finally:
        ctx.close()


# ---- 5. profiling --------------------------------------------------------------------------

FORWARD_STAGES = {"transform", "emit"}
ROUND_TRIP_STAGES = {"transform", "emit", "decode", "inverse", "rmse"}


def round_trip(ctx, B, cells, o):
    """wc_forward, wc_inverse, wc_rmse: every stage of ROUND_TRIP_STAGES."""
    ctx.forward(cells.data_ptr(), B.code, B.units, B.n, KEEP, o.pay.data_ptr(), B.cap, o.po.data_ptr(),
                o.kept.data_ptr())
    ctx.inverse(o.pay.data_ptr(), o.po.data_ptr(), B.units, B.n, o.out2.data_ptr())
    ctx.rmse(cells.data_ptr(), B.code, o.out2.data_ptr(), B.units, B.n, o.r2.data_ptr())


def test_profile_stages_counts_and_unchanged_results(wc, oracle):
    """Off: nothing is read.  On: wc_forward fills TRANSFORM and EMIT only
    (launches >= 1, finite ms > 0), wc_inverse and wc_rmse add DECODE, INVERSE
    and RMSE, a second read returns nothing, two identical call sequences count
    the same launches, and the bytes and cells equal those with profiling off."""
    import torch
    B = batch(wc, oracle, "base", np.float64)
    ctx = wc.capi.Context(0)
    try:
        cells = device_cells(torch, B)
        off, on = Outs(torch, B), Outs(torch, B)
        torch.cuda.synchronize()
        round_trip(ctx, B, cells, off)
        ctx.synchronize()
        assert ctx.profile_read() == {}
        ctx.profile_enable(True)
        ctx.forward(cells.data_ptr(), B.code, B.units, B.n, KEEP, on.pay.data_ptr(), B.cap, on.po.data_ptr(),
                    on.kept.data_ptr())
        ctx.synchronize()
        p = ctx.profile_read()
        assert set(p) == FORWARD_STAGES, p
        for ms, launches in p.values():
            assert launches >= 1 and math.isfinite(ms) and ms > 0.0, p
        assert ctx.profile_read() == {}
        ctx.inverse(on.pay.data_ptr(), on.po.data_ptr(), B.units, B.n, on.out2.data_ptr())
        ctx.rmse(cells.data_ptr(), B.code, on.out2.data_ptr(), B.units, B.n, on.r2.data_ptr())
        p = ctx.profile_read()  # waits for the last mark itself
        assert set(p) == {"decode", "inverse", "rmse"}, p
        for ms, launches in p.values():
            assert launches >= 1 and math.isfinite(ms) and ms > 0.0, p
        assert ctx.profile_read() == {}
        counts = []
        for _ in range(2):
            round_trip(ctx, B, cells, on)
            ctx.synchronize()
            p = ctx.profile_read()
            assert set(p) == ROUND_TRIP_STAGES, p
            counts.append({k: v[1] for k, v in p.items()})
        assert counts[0] == counts[1], counts
        ctx.profile_enable(False)
        round_trip(ctx, B, cells, off)
        ctx.synchronize()
        assert ctx.profile_read() == {}
        a, b = off.host(), on.host()
        for k in ("pay", "po", "kept", "out2", "r2"):
            assert a[k].tobytes() == b[k].tobytes(), k
        check_forward(B, b["pay"], b["po"], b["kept"], "profiling on")
        for i, u in enumerate(B.six()):
            assert same_cells(b["out2"][B.offs[i]:B.offs[i] + u["back"].size], u["back"]), (i, B.dims[i])
    finally:
        ctx.close()


def test_profile_times_fit_inside_the_callers_bracket(wc, oracle, capsys):
    """On a caller's stream the stage intervals are disjoint sub-intervals of the
    interval between two torch events that bracket the same calls, so their sum
    exceeds the bracket by timer granularity at most: marks * g, g the largest
    elapsed time of 20 event pairs recorded back to back with nothing between
    them, measured here."""
    import torch
    B = batch(wc, oracle, "base", np.float64)
    ctx = wc.capi.Context(0)
    s = torch.cuda.Stream()
    try:
        cells = device_cells(torch, B)
        o = Outs(torch, B)
        torch.cuda.synchronize()
        round_trip(ctx, B, cells, o)  # plan and scratch
        ctx.synchronize()
        ctx.set_stream(s.cuda_stream)
        ctx.profile_enable(True)
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            for a, b in pairs:
                a.record(s)
                b.record(s)
            e0.record(s)
            round_trip(ctx, B, cells, o)
            e1.record(s)
        s.synchronize()
        g = max(a.elapsed_time(b) for a, b in pairs)
        bracket = e0.elapsed_time(e1)
        p = ctx.profile_read()
        total, marks = sum(ms for ms, _ in p.values()), sum(k for _, k in p.values())
        with capsys.disabled():
            print("\nprofile bracket: stages %.6f ms in %d marks, bracket %.6f ms, g %.6f ms" % (total, marks, bracket, g))
        assert set(p) == ROUND_TRIP_STAGES, p
        assert g >= 0.0 and total <= bracket + marks * g, (total, bracket, marks, g)
    finally:
        ctx.set_stream(None)
        ctx.close()


def test_profile_read_raw_abi(wc, oracle):
    """wc_profile_read's nstages: 3 fills exactly three entries and leaves a fourth
    untouched; the marks of stages at or beyond nstages are dropped, not
    written; 0 with null arrays is WC_OK; negative is WC_ERR_INVALID."""
    import torch
    B = batch(wc, oracle, "header", np.float64)
    ctx = wc.capi.Context(0)
    L, h = ctx._L, ctx.handle
    try:
        cells = device_cells(torch, B)
        o = Outs(torch, B)
        torch.cuda.synchronize()
        ctx.profile_enable(True)
        round_trip(ctx, B, cells, o)
        ctx.synchronize()
        ms, cnt = (ctypes.c_double * 4)(-7.0, -7.0, -7.0, -7.0), (ctypes.c_uint32 * 4)(9, 9, 9, 9)
        assert L.wc_profile_read(h, ms, cnt, 3) == WC_OK
        assert all(cnt[i] >= 1 and ms[i] > 0.0 for i in range(3)), (list(ms), list(cnt))
        assert ms[3] == -7.0 and cnt[3] == 9
        assert ctx.profile_read() == {}  # INVERSE and RMSE were dropped with that read
        round_trip(ctx, B, cells, o)
        ctx.synchronize()
        assert L.wc_profile_read(h, None, None, 0) == WC_OK
        assert ctx.profile_read() == {}
        assert L.wc_profile_read(h, ms, cnt, -1) == WC_ERR_INVALID
        assert ms[3] == -7.0 and cnt[3] == 9
    finally:
        ctx.close()
