"""GPU: seeded random batches through the RMSE tolerance on the multi-level transform
(wc_forward_levels_tol and its _host form) against the numpy restatement of the
per-level rule (leveltol_rule.py).  Every comparison is bit or byte equality.

The batches are rule_fuzz.leveltol_case's (test_rule_fuzz_cpu.py runs seeds 0 and 1
through the host rule and proves their classes): modes_batches.levels_batch without
the units the mode refuses, at its own cell offsets (random gaps, every third unit at
an odd element offset, so that a level boundary falls at a random offset of a 16-byte
group), random 2-adic shapes and levels, NaN / inf / subnormal cells, and per unit a
tolerance of modes_batches.tol_batch's draw: 0, +inf or 10^U(-6, 3) x the unit's RMS.

Bar: test_gpu_leveltol.check_outputs (per-level thresh bits with 0.0f past L, bound
double bits, kept, the payload bytes of leveltol_rule.payload, slot offsets) and
check_regen (wc_inverse_levels of the payloads equals levels_ref.decode under
same_cells; no cell outside a unit is written).  Each seed runs under the default
options and one look-back option set chosen by the seed, with WC_OPT_TOL_SOLO_TILES 64
and 1; seed 0 under every look-back set and through the _host form in one run and in
runs of one unit.  WC_FUZZ_SEEDS=N soaks N seeds."""
import os

import numpy as np
import pytest

import rule_fuzz as RF
from test_gpu_fuzz import _OPTION_SETS
from test_gpu_leveltol import check_outputs, check_regen, forward
from test_gpu_modes_fuzz import LOOKBACK, options
from tol_rule import same_bits
from wavelet_compression_amd.capi import WC_MAX_LEVELS, WC_OPT_HOST_CHUNK, WC_OPT_TOL_SOLO_TILES

pytestmark = pytest.mark.gpu

_N = int(os.environ.get("WC_FUZZ_SEEDS", "0"))


def run(wc, ctx, B, what):
    d = forward(wc, ctx, B)
    check_outputs(B, d.read(), what)
    check_regen(ctx, B, d, what)


@pytest.mark.parametrize("solo", [64, 1])
@pytest.mark.parametrize("opts", ["default", "lookback"])
@pytest.mark.parametrize("seed", range(_N or 2))
def test_leveltol_random_batches(wc, ctx, oracle, seed, opts, solo):
    B = RF.leveltol_case(wc.capi, oracle, seed)
    name = LOOKBACK[seed % len(LOOKBACK)]
    pairs = (() if opts == "default" else _OPTION_SETS[name]) + ((WC_OPT_TOL_SOLO_TILES, solo),)
    with options(wc, ctx, pairs):
        run(wc, ctx, B, (seed, opts if opts == "default" else name, solo))


@pytest.mark.parametrize("opts", LOOKBACK)
def test_leveltol_option_paths(wc, ctx, oracle, opts):
    B = RF.leveltol_case(wc.capi, oracle, 0)
    with options(wc, ctx, _OPTION_SETS[opts]):
        run(wc, ctx, B, opts)


@pytest.mark.parametrize("chunk", [None, 1])
def test_leveltol_host_form(wc, ctx, oracle, chunk):
    """wc_forward_levels_tol_host on seed 0 in one run and in runs of one unit: the restatement's payloads,
    packed 24 + 8 kept bytes apart; thresholds and bounds."""
    B = RF.leveltol_case(wc.capi, oracle, 0)
    with options(wc, ctx, ((WC_OPT_HOST_CHUNK, chunk),) if chunk is not None else ()):
        payload, offs, kept, thresh, bound, _ = ctx.forward_levels_tol_host(B.cells, B.units, B.n, B.levels, B.tol,
                                                                           want_rmse=False)
    pos = 4
    for i in range(B.n):
        pay, k, th, bd = B.want[i]
        who = (chunk, i, B.dims[i], B.levels[i], B.tol[i])
        assert int(kept[i]) == k and int(offs[i]) == pos, who
        assert wc.capi.unit_payload(payload, offs, kept, i) == pay, who
        pos += 24 + 8 * k
        for l in range(WC_MAX_LEVELS):
            assert same_bits(float(thresh[i, l]), th[l] if l < B.levels[i] else 0.0, np.float32), (who, l + 1)
        assert same_bits(float(bound[i]), bd), who
    assert int(offs[B.n]) == pos - 4
