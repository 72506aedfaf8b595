"""GPU: seeded random batches through the size-budget mode
(wc_forward_levels_budget) against the numpy restatement (budget_rule.py).

The batches are modes_batches.levels_batch's (the pinned shapes, the NaN / inf
specials, random 2-adic shapes and levels, empty units, random gaps and odd
offsets) without the units the mode refuses (cells and an odd dimension).  Each
unit's budget is drawn from {0, c, c - 1, c + 1, a uniform rank}, c its
candidate count.  Bar: T, thresholds, kept counts and payload bytes equal the
restatement's, under the default options and under every look-back form."""
import os

import numpy as np
import pytest

import budget_rule as BR
import modes_batches as M
from test_gpu_budget import SENT_K, SENT_T, Dev
from test_gpu_fuzz import _OPTION_SETS
from test_gpu_modes_fuzz import LOOKBACK, options
from tol_rule import same_bits
from wavelet_compression_amd.capi import WC_MAX_LEVELS, WC_OPT_TOL_SOLO_TILES

pytestmark = pytest.mark.gpu

_N = int(os.environ.get("WC_FUZZ_SEEDS", "0"))
_cases = {}


class FuzzCase:
    def __init__(self, wc, oracle, seed):
        LB = M.levels_batch(oracle, seed)
        keep = [i for i, d in enumerate(LB.dims) if not (d[0] * d[1] * d[2] and (d[0] | d[1] | d[2]) & 1)]
        rng = np.random.default_rng(8500 + seed)
        self.dtype = LB.dtype
        self.dims = [LB.dims[i] for i in keep]
        self.levels = [LB.levels[i] for i in keep]
        self.n = len(keep)
        self.units, _, self.extent = wc.capi.make_units(self.dims, [LB.offsets[i] for i in keep], align=1)
        self.cells = np.zeros(max(self.extent, 1), self.dtype)
        self.budgets, self.want = [], []
        for u, i in enumerate(keep):
            b = LB.boxes[i]
            o = self.units[u].cell_offset
            self.cells[o:o + b.size] = b.ravel().astype(self.dtype)
            prep = BR.prepare(M.narrow(oracle, b, self.dtype), self.levels[u])
            c = len(prep[7])
            K = int(rng.choice([0, c, max(c - 1, 0), c + 1, int(rng.integers(0, c + 1))]))
            self.budgets.append(K)
            self.want.append(BR.payload_of(prep, K))
        tags = {t: i for t, i in LB.tags.items()}
        assert all(keep[u] == u for u in range(len(M.PINNED) + len(M.SPECIALS))) and set(M.SPECIAL_TAGS) <= set(tags)
        assert any(0 < K for K in self.budgets) and any(w[1] < K for w, K in zip(self.want, self.budgets))


def fuzz_case(wc, oracle, seed):
    if seed not in _cases:
        _cases[seed] = FuzzCase(wc, oracle, seed)
    return _cases[seed]


def run(wc, ctx, B, what):
    d = Dev(wc, B.units, B.n, B.cells)
    ctx.forward_levels_budget(d.cells.data_ptr(), d.code, B.units, B.n, B.levels, B.budgets, *d.out_args())
    ctx.synchronize()
    payloads, kept, off, thresh, key = d.read()
    for i in range(B.n):
        pay, k, T, th, _ = B.want[i]
        who = (what, i, B.dims[i], B.levels[i], B.budgets[i])
        assert int(key[i]) == T, (who, hex(int(key[i])), hex(T))
        for l in range(WC_MAX_LEVELS):
            assert same_bits(float(thresh[i, l]), th[l] if l < B.levels[i] else 0.0, np.float32), (who, l + 1)
        assert int(kept[i]) == k and k <= B.budgets[i], (who, int(kept[i]), k)
        assert payloads[i] == pay, who
    assert SENT_T not in thresh and (B.n == 0 or SENT_K not in key.tolist())


@pytest.mark.parametrize("solo_tiles", [64, 1])
@pytest.mark.parametrize("seed", range(_N or 2))
def test_budget_random_batches(wc, ctx, oracle, seed, solo_tiles):
    B = fuzz_case(wc, oracle, seed)
    with options(wc, ctx, [(WC_OPT_TOL_SOLO_TILES, solo_tiles)]):
        run(wc, ctx, B, (seed, solo_tiles))


@pytest.mark.parametrize("opts", LOOKBACK)
def test_budget_option_paths(wc, ctx, oracle, opts):
    B = fuzz_case(wc, oracle, 0)
    with options(wc, ctx, _OPTION_SETS[opts]):
        run(wc, ctx, B, opts)
