"""GPU: seeded random batches through the pair pipeline (wc_thin_budget /
wc_thin_thresh, wc_split_budget / wc_split_thresh, wc_merge) against the numpy
restatements (thin_rule.py, layers_rule.py).  Every comparison is byte equality.

The batches are pairs_fuzz.batch()'s (test_pairs_scale_cpu.py runs seeds 0 and 1
through the host rule): about 24 units of at most 2^15 cells and one of 65-70 pair
tiles, pair counts around the wave and the tile, heavy-tailed and overshooting
runs, surplus pairs, log-uniform and quantised value bits with the specials.  Per
seed: thinning and a split in both forms (test_gpu_thin.Dev.check and
test_gpu_layers.SplitDev.check: sentinels, slots, no byte outside a payload), the
merge of two layers in both orders (MergeDev.check), three layers merged in both
groupings on the device, and split(rest, K2) as the next layer merged back to
canon(P), each call reading the device buffers the call before it wrote.  Each seed
runs under the default options and under one look-back option set chosen by the
seed, with WC_OPT_TOL_SOLO_TILES 64 and 1.  WC_FUZZ_SEEDS=N soaks N seeds."""
import os

import numpy as np
import pytest

import decode_payloads as DP
import layers_rule as LR
import pairs_fuzz as PF
import pairs_scale as PS
from test_gpu_fuzz import _OPTION_SETS
from test_gpu_layers import MergeDev, SplitDev
from test_gpu_modes_fuzz import LOOKBACK, options
from test_gpu_thin import Dev as ThinDev
from wavelet_compression_amd.capi import WC_OPT_TOL_SOLO_TILES

pytestmark = pytest.mark.gpu

_N = int(os.environ.get("WC_FUZZ_SEEDS", "0"))
_cases = {}


class _Layers:
    """Two layers of a unit in the shape MergeDev reads a pair."""

    def __init__(self, u):
        self.name, self.dims, self.L, self.N = u.name, u.dims, u.L, u.N
        self.pay = [u.layers[0], u.layers[1]]
        self.live = tuple(LR.live_pairs(p)[4].size for p in self.pay)


class FuzzCase:
    def __init__(self, wc, seed):
        B = PF.batch(seed)
        rng = np.random.default_rng(17500 + seed)
        self.us, self.n, self.dims, self.levels = B.us, B.n, B.dims, B.levels
        self.units, _, self.extent = wc.capi.make_units(self.dims)
        self.buf, self.off = DP.payload_layout([u.payload for u in B.us], rng)
        th = np.stack([u.thresh for u in B.us])
        self.budget = PS.View(self, [u.K for u in B.us], np.zeros_like(th),
                              [(u.split[0], u.split[2], u.split[4], u.split[5], None) for u in B.us],
                              [u.split for u in B.us])
        self.thresh = PS.View(self, [0xFFFFFFFF] * B.n, th, [(u.tsplit[0], u.tsplit[2], 0, [], None) for u in B.us],
                              [u.tsplit for u in B.us])
        # the merge of layers 0 and 1, in test_gpu_layers.MergeCase's shape
        M = type("Merge", (), {})()
        M.ps, M.n, M.dims, M.levels, M.units = [_Layers(u) for u in B.us], B.n, self.dims, self.levels, self.units
        M.want = [u.merged01 for u in B.us]
        M.abuf, M.aoff = DP.payload_layout([u.layers[0] for u in B.us], rng)
        M.bbuf, M.boff = DP.payload_layout([u.layers[1] for u in B.us], rng)
        M.slot, o = [], 4
        for u in B.us:
            M.slot.append(o)
            o += 24 + 8 * u.N
        M.cap = o
        self.merge = M
        self.cbuf, self.coff = DP.payload_layout([u.layers[2] for u in B.us], rng)


def fuzz_case(wc, seed):
    if seed not in _cases:
        _cases[seed] = FuzzCase(wc, seed)
    return _cases[seed]


def _chains(wc, ctx, F, what):
    """Three layers in both groupings, and the next layer of a split merged back: a call's device outputs
    (payloads and offsets) are the next call's inputs."""
    import torch
    dev = torch.device("cuda", 0)
    n, units, levels = F.n, F.units, F.levels
    cap = wc.capi.payload_bound(units, n)

    alive = []  # every buffer lives until the sync: the calls are asynchronous, and a freed tensor's memory is reused

    def bufs(c):
        alive.append((torch.full((c,), 0xA5, dtype=torch.uint8, device=dev),
                      torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)))
        return alive[-1]

    def up(buf, off):
        alive.append((torch.from_numpy(buf).to(dev), torch.from_numpy(off.view(np.int64)).to(dev)))
        return alive[-1]

    def merge(a, b):
        out = bufs(cap)
        torch.cuda.synchronize()  # the fills run on torch's stream, the context on its own
        ctx.merge(a[0].data_ptr(), a[1].data_ptr(), b[0].data_ptr(), b[1].data_ptr(), units, n, levels, out[0].data_ptr(),
                  cap, out[1].data_ptr(), out[2].data_ptr())
        return out

    def split(p, K):
        bcap, rcap = wc.capi.split_bound(units, n, K)
        base, rest = bufs(bcap), bufs(rcap)
        torch.cuda.synchronize()
        ctx.split_budget(p[0].data_ptr(), p[1].data_ptr(), units, n, levels, K, base[0].data_ptr(), bcap, base[1].data_ptr(),
                         base[2].data_ptr(), rest[0].data_ptr(), rcap, rest[1].data_ptr(), rest[2].data_ptr())
        return base, rest

    def read(b):
        pay, o, cnt = b[0].cpu().numpy(), b[1].cpu().numpy().view(np.uint64), b[2].cpu().numpy().view(np.uint32)
        return [wc.capi.unit_payload(pay, o, cnt, i) for i in range(n)]

    M = F.merge
    l0, l1, l2 = up(M.abuf, M.aoff), up(M.bbuf, M.boff), up(F.cbuf, F.coff)
    left = merge(merge(l0, l1), l2)
    right = merge(l0, merge(l1, l2))
    base, rest = split(up(F.buf, F.off), F.budget.K)
    b2, r2 = split(rest, [u.K2 for u in F.us])
    back = merge(base, merge(r2, b2))
    ctx.synchronize()
    got = [read(x) for x in (left, right, b2, r2, back)]
    for i, u in enumerate(F.us):
        who = (what, i, u.name, u.dims, u.L, u.K, u.K2)
        assert got[0][i] == got[1][i] == u.merged, who
        assert (got[2][i], got[3][i]) == u.split2[:2], who
        assert got[4][i] == u.canon, who
    assert left[0].cpu().numpy().tobytes() == right[0].cpu().numpy().tobytes(), what


def run(wc, ctx, F, what):
    for V, budget in ((F.budget, True), (F.thresh, False)):
        d = ThinDev(wc, V, budget)
        d.run(ctx)
        ctx.synchronize()
        d.check((what, "thin", budget))
        d = SplitDev(wc, V, budget)
        d.run(ctx)
        ctx.synchronize()
        d.check(V.split, (what, "split", budget))
    for swap in (False, True):
        d = MergeDev(wc, F.merge, one_buffer=swap)
        d.run(ctx, swap=swap)
        ctx.synchronize()
        d.check((what, "merge", swap))
    _chains(wc, ctx, F, what)


@pytest.mark.parametrize("solo", [64, 1])
@pytest.mark.parametrize("opts", ["default", "lookback"])
@pytest.mark.parametrize("seed", range(_N or 2))
def test_pairs_random_batches(wc, ctx, seed, opts, solo):
    F = fuzz_case(wc, seed)
    name = LOOKBACK[seed % len(LOOKBACK)]
    pairs = (() if opts == "default" else _OPTION_SETS[name]) + ((WC_OPT_TOL_SOLO_TILES, solo),)
    with options(wc, ctx, pairs):
        run(wc, ctx, F, (seed, opts if opts == "default" else name, solo))
