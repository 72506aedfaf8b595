"""GPU: seeded random batches and the probe-tile edges through the pointwise error
bound (wc_forward_levels_maxerr, its _host form, wc_maxerr, wc_maxerr_host) against
the numpy restatement (maxerr_rule.py).  Every comparison is bit or byte equality.

The random batches are rule_fuzz.maxerr_case's (test_rule_fuzz_cpu.py runs seeds 0 and
1 through the host rule and proves their classes): modes_batches.levels_batch without
the units the mode refuses, at its own cell offsets, so that units start off a
2 * sizeof(T) boundary and the probe kernel loads their cells one by one; seed parity
picks fp64 / fp32.  A unit's bound is 0, +inf, a fraction of its max |x|, E = err(b)
of a random bin, where `err(b) <= E` holds with equality, or the double just below.
The tile units are maxerr_tiles.py's: every admissible clip of a probe tile on every
axis and units whose error comes from one chosen tile alone, in four calls whose
largest L is 1, 2, 3 and 4 (the 16 x 8 x 32 forms and the 16 x 16 x 32 one), in both
cell types, packed at 4-element alignment and with every unit at an odd offset.

Bar: test_gpu_maxerr.check_outputs (thresh float bits, err double bits, kept, payload
bytes, slot offsets, thresh == 0 or err <= E); under the default options also the
payloads decoded by wc_inverse_levels, on which maxerr_rule.max_abs in numpy, wc_maxerr
and wc_maxerr_host give the d_err bits again (the units sit at odd offsets and their
last flat tile is partial), and no cell outside a unit is written.  Each seed runs
under the default options and one look-back option set chosen by the seed, with
WC_OPT_TOL_SOLO_TILES 64 and 1; seed 0 under every look-back set and through the _host
form in one run and in runs of one unit.  WC_FUZZ_SEEDS=N soaks N seeds."""
import os

import numpy as np
import pytest

import maxerr_rule as MR
import rule_fuzz as RF
from test_gpu_fuzz import _OPTION_SETS
from test_gpu_maxerr import SENT_E, Dev, check_outputs
from test_gpu_modes_fuzz import LOOKBACK, options
from tol_rule import same_bits
from wavelet_compression_amd.capi import WC_OPT_HOST_CHUNK, WC_OPT_TOL_SOLO_TILES

pytestmark = pytest.mark.gpu

_N = int(os.environ.get("WC_FUZZ_SEEDS", "0"))


def run(wc, ctx, B, what, decode=False):
    import torch
    d = Dev(wc, B)
    ctx.forward_levels_maxerr(d.cells.data_ptr(), d.code, B.units, B.n, B.levels, B.E, *d.out_args())
    ctx.synchronize()
    got = d.read()
    check_outputs(B, got, what)
    if not decode:
        return
    _, _, _, thresh, err = got
    ctx.inverse_levels(d.pay.data_ptr(), d.off.data_ptr(), B.units, B.n, B.levels, d.out.data_ptr())
    ctx.synchronize()
    out = d.out.cpu().numpy()
    for i, x in enumerate(B.x):
        o = B.units[i].cell_offset
        e = MR.max_abs(x, out[o:o + x.size])
        assert same_bits(e, float(err[i])), (what, i, B.dims[i], e, float(err[i]))
        assert thresh[i] == 0.0 or e <= B.E[i], (what, i, e, B.E[i])
    assert np.all(out[~B.owned] == -77.0), (what, "written outside the units")
    again = torch.full((B.n,), SENT_E, dtype=torch.float64, device=d.pay.device)
    torch.cuda.synchronize()
    ctx.maxerr(d.cells.data_ptr(), d.code, d.out.data_ptr(), B.units, B.n, again.data_ptr())
    ctx.synchronize()
    assert again.cpu().numpy().tobytes() == err.tobytes(), what
    assert ctx.maxerr_host(B.cells, out, B.units, B.n).tobytes() == err.tobytes(), what


@pytest.mark.parametrize("solo", [64, 1])
@pytest.mark.parametrize("opts", ["default", "lookback"])
@pytest.mark.parametrize("seed", range(_N or 2))
def test_maxerr_random_batches(wc, ctx, oracle, seed, opts, solo):
    B = RF.maxerr_case(wc.capi, oracle, seed)
    name = LOOKBACK[seed % len(LOOKBACK)]
    pairs = (() if opts == "default" else _OPTION_SETS[name]) + ((WC_OPT_TOL_SOLO_TILES, solo),)
    with options(wc, ctx, pairs):
        run(wc, ctx, B, (seed, opts if opts == "default" else name, solo), decode=opts == "default" and solo == 64)


@pytest.mark.parametrize("opts", LOOKBACK)
def test_maxerr_option_paths(wc, ctx, oracle, opts):
    B = RF.maxerr_case(wc.capi, oracle, 0)
    with options(wc, ctx, _OPTION_SETS[opts]):
        run(wc, ctx, B, opts)


@pytest.mark.parametrize("chunk", [None, 1])
def test_maxerr_host_form(wc, ctx, oracle, chunk):
    """wc_forward_levels_maxerr_host on seed 0 in one run and in runs of one unit: the restatement's payloads,
    packed 24 + 8 kept bytes apart; thresholds and errors."""
    B = RF.maxerr_case(wc.capi, oracle, 0)
    with options(wc, ctx, ((WC_OPT_HOST_CHUNK, chunk),) if chunk is not None else ()):
        payload, offs, kept, thresh, err, _ = ctx.forward_levels_maxerr_host(B.cells, B.units, B.n, B.levels, B.E,
                                                                            want_rmse=False)
    pos = 4
    for i in range(B.n):
        pay, k, th, e, b = B.want[i]
        who = (chunk, i, B.dims[i], B.levels[i], B.E[i], b)
        assert int(kept[i]) == k and int(offs[i]) == pos, who
        assert wc.capi.unit_payload(payload, offs, kept, i) == pay, who
        pos += 24 + 8 * k
        assert same_bits(float(thresh[i]), float(th), np.float32) and same_bits(float(err[i]), e), who
        assert thresh[i] == 0.0 or err[i] <= B.E[i], who
    assert int(offs[B.n]) == pos - 4


@pytest.mark.parametrize("layout", ["aligned", "odd"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("maxl", [1, 2, 3, 4])
def test_probe_tile_edges(wc, ctx, oracle, maxl, dtype, layout):
    """The call's largest L is maxl: maxl = 4 runs every unit of maxerr_tiles.py under the 16 x 16 x 32 tile,
    the others the units of at most maxl levels under 16 x 8 x 32."""
    B = RF.tiles_case(wc.capi, oracle, maxl, dtype, layout == "odd")
    assert max(B.levels) == maxl
    run(wc, ctx, B, (maxl, dtype.__name__, layout), decode=True)
