"""GPU: the decoders on crafted payloads (tests/decode_payloads.py): pair counts
at the edges of the scan and past the launched tiles, positions at the edges of
the box, of its rows and of a region's index map, run sums past 2^31 - 1 and
2^32, value bits no encoder emits; and seeded mixes of them with heavy-tailed
random runs.  Every entry point that decodes payloads, against its CPU
reference:

  wc_inverse, wc_inverse_rmse, wc_inverse_host     oracle.decompress_payload
  wc_inverse_levels, wc_inverse_levels_host        levels_ref.decode
  wc_inverse_coarse (every r in 0..L)              coarse_ref.decode
  wc_inverse_region (r = 0, 1; whole box, a slab   region_ref.decode
    per axis, the far corner block)

The rule for a run sum past 2^31 - 1 is the project's (wc_pairscan.h; the
reference's int index is undefined there): positions never decrease, every pair
at or past ncoeff is dropped; the oracle's 64-bit index implements it
(tests/test_decode_payloads_cpu.py).

Per call: cells bit for bit, a NaN matching any NaN (test_gpu_fuzz.same_cells);
the sentinel between the output units untouched; no error at wc_synchronize;
the payload and offset buffers as they were uploaded.  Before each call the
same entry point decodes an all-kept payload of the same units, so that a tile
that never runs leaves stale coefficients, not zeros.  The RMSE of
wc_inverse_rmse: test_gpu_fuzz's bound, max(1e-12, (n + 4) 2^-53) relative.
"""
import numpy as np
import pytest

import coarse_ref as C
import decode_payloads as DP
import levels_ref as LR
import pack_rule as PR
import region_ref as G
from test_gpu_fuzz import same_cells

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
BATCH = 60
_REF = {}  # (unit name, kind, r, region) -> the reference cells, computed once and left unchanged


def reference(oracle, u, kind, r=0, region=None):
    key = (u.name, kind, r, region)
    if key not in _REF:
        if u.ncoeff == 0:
            _REF[key] = np.zeros(0, np.float32)
        elif kind == "inverse":
            _REF[key] = oracle.decompress_payload(u.payload)
        elif kind == "levels":
            _REF[key] = LR.decode(u.payload)[0]
        elif kind == "coarse":
            _REF[key] = C.decode(u.payload, r)
        else:
            _REF[key] = G.decode(u.payload, r, region)
        _REF[key].flags.writeable = False
    return _REF[key]


def whole(u):
    return (0, 0, 0) + u.dims


class Batch:
    """Entries (unit, r, region) of one call: the payloads in one buffer in
    another order with gaps at offsets 0 and 4 (mod 8), the output units with
    gaps and odd offsets, an all-kept payload per entry in the standard layout,
    the reference cells."""

    def __init__(self, wc, oracle, entries, kind, seed):
        rng = np.random.default_rng(7000 + seed)
        self.kind, self.n = kind, len(entries)
        self.entries = [(u, r, whole(u) if g is None else tuple(g)) for u, r, g in entries]
        self.units_ = [u for u, _, _ in self.entries]
        self.levels = [u.L for u in self.units_]
        self.reduce = [r for _, r, _ in self.entries]
        self.regions = [g if u.ncoeff else (0, 0, 0, 0, 0, 0) for u, _, g in self.entries]
        self.cdims = [G.out_dims(g, r) for g, r in zip(self.regions, self.reduce)]
        if kind in ("inverse", "levels"):  # (a unit without cells keeps its dimensions)
            self.cdims = [u.dims for u in self.units_]
        self.offs, self.extent = DP.cell_layout([w * h * d for w, h, d in self.cdims], rng)
        self.out_units, _, _ = wc.capi.make_units(self.cdims, self.offs)
        # the full units: the output units themselves where the call has no others
        self.units = self.out_units if kind in ("inverse", "levels") else wc.capi.make_units([u.dims for u in self.units_])[0]
        self.buf, self.off = DP.payload_layout([u.payload for u in self.units_], rng)
        kept = [PR.standard(*u.dims, u.L, np.zeros(u.ncoeff, np.uint32), np.full(u.ncoeff, 0x40F00000, np.uint32))
                for u in self.units_]  # every coefficient 7.5
        self.dirty_off, cap = PR.payload_slots([u.dims for u in self.units_])
        self.dirty = np.zeros(cap + 8, np.uint8)
        for o, p in zip(self.dirty_off, kept):
            self.dirty[o:o + len(p)] = np.frombuffer(p, np.uint8)
        self.dirty_off = np.array(self.dirty_off + [0], np.uint64)[:max(self.n, 1)]
        self.want = [reference(oracle, u, kind, r, g if kind == "region" else None) for u, r, g in self.entries]
        self.owned = np.zeros(self.extent, bool)
        for o, (w, h, d) in zip(self.offs, self.cdims):
            self.owned[o:o + w * h * d] = True

    def check(self, cells, what):
        assert cells.size == self.extent
        for i, (u, r, g) in enumerate(self.entries):
            o, w = self.offs[i], self.want[i]
            assert w.shape == tuple(reversed(self.cdims[i])) or w.size == 0
            assert same_cells(cells[o:o + w.size], w.ravel()), (what, self.kind, i, u.name, r, g)
        assert np.all(cells[~self.owned] == SENTINEL), (what, self.kind)  # nothing written outside the units


class Dev:
    def __init__(self, b):
        import torch
        self.dev = torch.device("cuda", 0)
        self.pay, self.off = torch.from_numpy(b.buf).to(self.dev), torch.from_numpy(b.off.view(np.int64)).to(self.dev)
        self.dpay = torch.from_numpy(b.dirty).to(self.dev)
        self.doff = torch.from_numpy(b.dirty_off.view(np.int64)).to(self.dev)
        self.scratch = torch.empty(b.extent, dtype=torch.float32, device=self.dev)
        torch.cuda.synchronize()

    def fresh(self, b):
        import torch
        out = torch.full((b.extent,), SENTINEL, dtype=torch.float32, device=self.dev)
        torch.cuda.synchronize()  # the fill runs on torch's stream, the context on its own
        return out

    def unchanged(self, b):
        return self.pay.cpu().numpy().tobytes() == b.buf.tobytes() and \
            self.off.cpu().numpy().tobytes() == b.off.tobytes()


def call(ctx, b, pay, off, out):
    """The batch's entry point (device form)."""
    if b.kind == "inverse":
        ctx.inverse(pay, off, b.units, b.n, out)
    elif b.kind == "levels":
        ctx.inverse_levels(pay, off, b.units, b.n, b.levels, out)
    elif b.kind == "coarse":
        ctx.inverse_coarse(pay, off, b.units, b.n, b.levels, b.reduce, b.out_units, out)
    else:
        ctx.inverse_region(pay, off, b.units, b.n, b.levels, b.reduce, b.regions, b.out_units, out)


def run_device(ctx, b, d, what):
    """Dirty the scratch, decode into a sentinel-filled output, check everything."""
    call(ctx, b, d.dpay.data_ptr(), d.doff.data_ptr(), d.scratch.data_ptr())
    out = d.fresh(b)
    call(ctx, b, d.pay.data_ptr(), d.off.data_ptr(), out.data_ptr())
    ctx.synchronize()
    b.check(out.cpu().numpy(), what)
    assert d.unchanged(b), what


def run_rmse(wc, ctx, oracle, b, d, dtype, what):
    """wc_inverse_rmse against arbitrary finite originals."""
    import torch
    rng = np.random.default_rng(b.extent)
    orig = (rng.standard_normal(b.extent) * 10.0 ** rng.uniform(-3, 3, b.extent)).astype(dtype)
    code = wc.capi.WC_F64 if dtype == np.float64 else wc.capi.WC_F32
    dorig = torch.from_numpy(orig).to(d.dev)
    rmse = torch.full((max(b.n, 1),), -1.0, dtype=torch.float64, device=d.dev)
    ctx.inverse(d.dpay.data_ptr(), d.doff.data_ptr(), b.units, b.n, d.scratch.data_ptr())
    out = d.fresh(b)
    ctx.inverse_rmse(d.pay.data_ptr(), d.off.data_ptr(), b.units, b.n, dorig.data_ptr(), code, out.data_ptr(),
                     rmse.data_ptr())
    ctx.synchronize()
    b.check(out.cpu().numpy(), (what, "rmse", dtype.__name__))
    assert d.unchanged(b), what
    E = rmse.cpu().numpy()
    for i, (u, _, _) in enumerate(b.entries):
        if u.ncoeff == 0:
            continue
        W, H, D = u.dims
        o = orig[b.offs[i]:b.offs[i] + u.ncoeff].reshape(D, H, W)
        o32 = oracle.narrow(o) if dtype == np.float64 else o
        with np.errstate(all="ignore"):
            ref = oracle.rmse(o32, b.want[i])
        if np.isnan(ref):
            assert np.isnan(E[i]), (what, i, u.name, E[i])
        elif np.isinf(ref):
            assert E[i] == ref, (what, i, u.name, E[i], ref)
        else:
            tol = max(1e-12, (u.ncoeff + 4) * 2.0 ** -53)
            assert abs(E[i] - ref) <= tol * abs(ref), (what, i, u.name, E[i], ref)


def run_host(wc, ctx, b, what):
    """The host forms in several pipelined runs."""
    fn = {"inverse": lambda p, o, out: ctx.inverse_host(p, o, b.units, b.n, b.extent, out=out),
          "levels": lambda p, o, out: ctx.inverse_levels_host(p, o, b.units, b.n, b.extent, levels=b.levels, out=out)}[b.kind]
    before = ctx.get_option(wc.capi.WC_OPT_HOST_CHUNK)
    ctx.set_option(wc.capi.WC_OPT_HOST_CHUNK, 1 << 16)  # two 32^3 units to a run: up to 16 runs a batch
    try:
        fn(b.dirty, b.dirty_off[:b.n], np.empty(b.extent, np.float32))
        pay, off = b.buf.copy(), b.off.copy()
        cells = fn(pay, off[:b.n], np.full(b.extent, SENTINEL, np.float32))
    finally:
        ctx.set_option(wc.capi.WC_OPT_HOST_CHUNK, before)
    b.check(cells, (what, "host"))
    assert pay.tobytes() == b.buf.tobytes() and off.tobytes() == b.off.tobytes()


def chunks(items, size=BATCH):
    return [items[a:a + size] for a in range(0, len(items), size)]


def rix_shape(u):
    W, H, D = u.dims
    return u.ncoeff > 0 and W % 2 == 0 and H % 2 == 0 and D % 8 == 0


CRAFTED = DP.crafted()
# one level: the row-indexable boxes first (their batches take wc_inverse_rmse's fused form)
ONE_LEVEL = chunks(sorted((u for u in CRAFTED if u.L == 1), key=lambda u: not rix_shape(u)))
ANY_LEVEL = chunks(list(CRAFTED))
CUBES = [u for u in CRAFTED if u.dims == DP.CUBE]
COARSE = chunks([(u, r, None) for u in CUBES for r in range(u.L + 1)])
REGION = chunks([(u, r, g) for u in CUBES for r in (0, 1) for g in DP.regions_of(DP.CUBE, u.L)])


@pytest.mark.parametrize("rows", (1, 0))
@pytest.mark.parametrize("k", range(len(ONE_LEVEL)))
def test_inverse(wc, ctx, oracle, k, rows):
    """wc_inverse at the defaults and with the dense decode for every unit."""
    b = Batch(wc, oracle, [(u, 0, None) for u in ONE_LEVEL[k]], "inverse", k)
    before = ctx.get_option(wc.capi.WC_OPT_INVERSE_ROWS)
    ctx.set_option(wc.capi.WC_OPT_INVERSE_ROWS, rows)
    try:
        run_device(ctx, b, Dev(b), ("inverse", k, rows))
    finally:
        ctx.set_option(wc.capi.WC_OPT_INVERSE_ROWS, before)


@pytest.mark.parametrize("k", range(len(ONE_LEVEL)))
def test_inverse_rmse_and_host(wc, ctx, oracle, k):
    b = Batch(wc, oracle, [(u, 0, None) for u in ONE_LEVEL[k]], "inverse", 100 + k)
    d = Dev(b)
    for dtype in (np.float64, np.float32):
        run_rmse(wc, ctx, oracle, b, d, dtype, ("inverse_rmse", k))
    run_host(wc, ctx, b, ("inverse_host", k))


@pytest.mark.parametrize("k", range(len(ANY_LEVEL)))
def test_inverse_levels(wc, ctx, oracle, k):
    b = Batch(wc, oracle, [(u, 0, None) for u in ANY_LEVEL[k]], "levels", 200 + k)
    run_device(ctx, b, Dev(b), ("inverse_levels", k))
    run_host(wc, ctx, b, ("inverse_levels_host", k))


@pytest.mark.parametrize("k", range(len(COARSE)))
def test_inverse_coarse(wc, ctx, oracle, k):
    b = Batch(wc, oracle, COARSE[k], "coarse", 300 + k)
    run_device(ctx, b, Dev(b), ("inverse_coarse", k))


@pytest.mark.parametrize("k", range(len(REGION)))
def test_inverse_region(wc, ctx, oracle, k):
    b = Batch(wc, oracle, REGION[k], "region", 400 + k)
    run_device(ctx, b, Dev(b), ("inverse_region", k))


def test_the_batches_hold_every_class():
    """What the parametrised tests above decode: every crafted unit, each 32^3 unit
    at every r and over every region; no batch above 60 units."""
    assert {u.name for c in ONE_LEVEL for u in c} == {u.name for u in CRAFTED if u.L == 1}
    assert sum(len(c) for c in ANY_LEVEL) == len(CRAFTED)
    assert {(u.name, r) for c in COARSE for u, r, _ in c} == {(u.name, r) for u in CUBES for r in range(u.L + 1)}
    assert len({(u.name, r, g) for c in REGION for u, r, g in c}) == 10 * len(CUBES)
    assert all(len(c) <= BATCH for c in ONE_LEVEL + ANY_LEVEL + COARSE + REGION)
    assert all(rix_shape(u) for u in ONE_LEVEL[0]) and {L for u in CUBES for L in [u.L]} == {1, 2, 3}
    built = {u.cls for u in CRAFTED}
    assert built >= set(DP.ALL_CLASSES) - {"levels:2", "levels:3"}


def every_entry_point(wc, ctx, oracle, units, seed, what):
    """`units` (any mix) through every entry point that admits them, in batches of at most 60."""
    rng = np.random.default_rng(9000 + seed)
    one = [u for u in units if u.L == 1]
    for j, c in enumerate(chunks(one)):
        b = Batch(wc, oracle, [(u, 0, None) for u in c], "inverse", seed + j)
        d = Dev(b)
        run_device(ctx, b, d, (what, "inverse", j))
        run_rmse(wc, ctx, oracle, b, d, np.float64 if (seed + j) % 2 == 0 else np.float32, (what, j))
        run_host(wc, ctx, b, (what, "inverse_host", j))
    for j, c in enumerate(chunks(list(units))):
        b = Batch(wc, oracle, [(u, 0, None) for u in c], "levels", seed + 10 + j)
        run_device(ctx, b, Dev(b), (what, "inverse_levels", j))
        run_host(wc, ctx, b, (what, "inverse_levels_host", j))
    # the coarse and region decoders: boxes whose dimensions 2^L divides; a random r, a random aligned region
    able = [u for u in units if u.ncoeff and (u.dims[0] | u.dims[1] | u.dims[2]) & ((1 << u.L) - 1) == 0]
    coarse, region = [], []
    for u in able:
        coarse.append((u, int(rng.integers(0, u.L + 1)), None))
        m = 1 << u.L
        g0 = [int(rng.integers(0, n // m)) * m for n in u.dims]
        ge = [int(rng.integers(1, (n - o) // m + 1)) * m for n, o in zip(u.dims, g0)]
        region.append((u, int(rng.integers(0, u.L + 1)), None if rng.random() < 0.3 else tuple(g0 + ge)))
    for kind, entries in (("coarse", coarse), ("region", region)):
        for j, c in enumerate(chunks(entries)):
            b = Batch(wc, oracle, c, kind, seed + 20 + j)
            run_device(ctx, b, Dev(b), (what, kind, j))


@pytest.mark.parametrize("seed", DP.FUZZ_SEEDS)
def test_fuzz_batches(wc, ctx, oracle, seed):
    every_entry_point(wc, ctx, oracle, DP.fuzz_batch(seed), seed, ("fuzz", seed))


# Library options the decoders must give the same cells under (include/wavelet_amd.h wc_set_option)
_OPTION_SETS = {
    "tickets": (("WC_OPT_TICKETS", 1),),
    "reversed_tiles": (("WC_OPT_REVERSE_TILES", 1),),
    "spin_limit_1": (("WC_OPT_SPIN_LIMIT", 1),),
    "reversed_spin_1": (("WC_OPT_REVERSE_TILES", 1), ("WC_OPT_SPIN_LIMIT", 1)),
    "small_rix_tiles": (("WC_OPT_RIX_LDS", 1024), ("WC_OPT_RIX_TX", 0)),
    "two_groups": (("WC_OPT_INV_GROUPS", 2),),
}
HARD = [u for u in CRAFTED if DP.is_overshoot(u) or DP.is_surplus(u)]


@pytest.mark.parametrize("part", ("fuzz", "overshoot_surplus"))
@pytest.mark.parametrize("opts", sorted(_OPTION_SETS))
def test_option_legs(wc, ctx, oracle, opts, part):
    """One fuzz seed, and the overshoot and surplus classes, under each option set;
    the options restored afterwards."""
    keys = [(getattr(wc.capi, name), v) for name, v in _OPTION_SETS[opts]]
    before = [(k, ctx.get_option(k)) for k, _ in keys]
    for k, v in keys:
        ctx.set_option(k, v)
    try:
        every_entry_point(wc, ctx, oracle, DP.fuzz_batch(1) if part == "fuzz" else HARD, 50, (opts, part))
    finally:
        for k, v in before:
            ctx.set_option(k, v)
