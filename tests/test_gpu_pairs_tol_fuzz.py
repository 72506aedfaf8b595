"""GPU: seeded random payloads through thinning and splitting to an RMSE tolerance in
the compressed domain (wc_thin_tol / wc_split_tol and their _host forms) against the
numpy restatement (thin_tol_rule.py).  Every comparison is byte equality.

The units are pairs_fuzz.tol_batch's (test_rule_fuzz_cpu.py runs seeds 0 and 1 through
the host rule and proves their classes): of each pairs_fuzz.batch(seed) the units the
calls take, with pair counts at 63..65 and 4095..4097, heavy-tailed runs that overshoot
N, surplus pairs, quantised magnitudes whose bins fill with ties, NaN / inf / +-0
pairs, and per unit a tolerance of 0, +inf or 10^U(-3, 0.5) x the payload's weighted
RMS.  The bin counts follow from the pairs and the box: a pair past N, a NaN pair or a
tie miscounted moves the stop.

Bar: test_gpu_thin_tol.Dev.check (bytes, kept, thresh bits, bound bits, offsets, slots,
no byte outside a payload, the input unwritten); for the split, wc_merge(base, rest) on
the device, reading the buffers the split wrote, equals layers_rule.canon(P).  Each
seed runs under the default options and one look-back option set chosen by the seed,
with WC_OPT_TOL_SOLO_TILES 64 and 1; seed 0 through the _host forms in one run and in
several.  WC_FUZZ_SEEDS=N soaks N seeds."""
import os

import numpy as np
import pytest

import decode_payloads as DP
import pairs_fuzz as PF
import thin_tol_rule as TT
from test_gpu_fuzz import _OPTION_SETS
from test_gpu_modes_fuzz import LOOKBACK, options
from test_gpu_thin_tol import Dev
from wavelet_compression_amd.capi import WC_MAX_LEVELS, WC_OPT_HOST_CHUNK, WC_OPT_TOL_SOLO_TILES

pytestmark = pytest.mark.gpu

_N = int(os.environ.get("WC_FUZZ_SEEDS", "0"))
_cases = {}


class FuzzCase:
    """pairs_fuzz.tol_batch(seed) in the shape test_gpu_thin_tol.Dev reads a batch."""

    def __init__(self, wc, seed):
        T = PF.tol_batch(seed)
        self.us, self.n, self.dims, self.levels, self.tol = T.us, T.n, T.dims, T.levels, T.tol
        self.want, self.split = T.want, T.split
        self.buf, self.off = DP.payload_layout([u.payload for u in T.us], np.random.default_rng(17600 + seed))
        self.units, _, self.extent = wc.capi.make_units(self.dims)
        self.slot, o = [], 4
        for u in self.us:
            self.slot.append(o)
            o += 24 + 8 * u.N
        self.bound = o


def fuzz_case(wc, seed):
    if seed not in _cases:
        _cases[seed] = FuzzCase(wc, seed)
    return _cases[seed]


def run(wc, ctx, C, what):
    import torch
    t, s = Dev(wc, C, False), Dev(wc, C, True)
    t.run(ctx)
    s.run(ctx)
    merged = torch.full((C.bound,), 0xA5, dtype=torch.uint8, device=t.pay.device)
    moff = torch.zeros(C.n + 1, dtype=torch.int64, device=t.pay.device)
    mcnt = torch.zeros(C.n, dtype=torch.int32, device=t.pay.device)
    torch.cuda.synchronize()  # the fills run on torch's stream, the context on its own
    ctx.merge(s.out[0].data_ptr(), s.ooff[0].data_ptr(), s.out[1].data_ptr(), s.ooff[1].data_ptr(), C.units, C.n,
              C.levels, merged.data_ptr(), C.bound, moff.data_ptr(), mcnt.data_ptr())
    ctx.synchronize()
    t.check((what, "thin"))
    s.check((what, "split"))
    m, mo, mk = merged.cpu().numpy(), moff.cpu().numpy().view(np.uint64), mcnt.cpu().numpy().view(np.uint32)
    for i, u in enumerate(C.us):
        assert wc.capi.unit_payload(m, mo, mk, i) == u.canon, (what, "merge", i, u.name, u.dims, u.L, u.tol)


@pytest.mark.parametrize("solo", [64, 1])
@pytest.mark.parametrize("opts", ["default", "lookback"])
@pytest.mark.parametrize("seed", range(_N or 2))
def test_pairs_tol_random_batches(wc, ctx, seed, opts, solo):
    C = fuzz_case(wc, seed)
    name = LOOKBACK[seed % len(LOOKBACK)]
    pairs = (() if opts == "default" else _OPTION_SETS[name]) + ((WC_OPT_TOL_SOLO_TILES, solo),)
    with options(wc, ctx, pairs):
        run(wc, ctx, C, (seed, opts if opts == "default" else name, solo))


@pytest.mark.parametrize("chunk", [None, 1 << 12])
@pytest.mark.parametrize("split", [False, True])
def test_pairs_tol_host_forms(wc, ctx, split, chunk):
    """wc_thin_tol_host / wc_split_tol_host on seed 0, in one run and in several: the restatement's bytes packed
    24 + 8 pairs bytes apart from 4, thresholds and bounds; with the levels from the headers and given."""
    C = fuzz_case(wc, 0)
    assert sum(u.N for u in C.us) > 2 << 12
    with options(wc, ctx, ((WC_OPT_HOST_CHUNK, chunk),) if chunk is not None else ()):
        for levels in (None, C.levels):
            if split:
                base, boff, kept, rest, roff, rp, th, bound = ctx.split_tol_host(C.buf, C.off, C.units, C.n, C.tol, levels)
                sides = [(base, boff, kept, [w[0] for w in C.want]), (rest, roff, rp, [s[1] for s in C.split])]
            else:
                out, off, kept, th, bound = ctx.thin_tol_host(C.buf, C.off, C.units, C.n, C.tol, levels)
                sides = [(out, off, kept, [w[0] for w in C.want])]
            for out, off, cnt, pays in sides:
                o = 4
                for i, u in enumerate(C.us):
                    k = (len(pays[i]) - 20) // 8
                    assert int(off[i]) == o and int(cnt[i]) == k, (i, u.name)
                    assert out[o:o + len(pays[i])].tobytes() == pays[i], (i, u.name)
                    o += 24 + 8 * k if i + 1 < C.n else 20 + 8 * k
                assert int(off[C.n]) == o
            for i, u in enumerate(C.us):
                want = TT.th_bits(list(C.want[i][2]) + [0.0] * (WC_MAX_LEVELS - u.L))
                assert TT.th_bits(th[i]) == want and TT.f64_bits(bound[i]) == TT.f64_bits(C.want[i][3]), (i, u.name)
