"""RMSE-tolerance mode without a GPU (include/wavelet_amd.h): the host-only
selection rule wc_tol_threshold against its numpy restatement (tol_rule.py),
bit for bit in the threshold and the bound; the rule end to end through the
CPU oracle (transform, bins, threshold, payload, reconstruction: the actual
RMSE stays within the tolerance); the CLI's `rmse=` parameter checks."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tol_rule import FLOOR, FLT_MAX, HIST_BINS, MARGIN, field, same_bits, tol_rule

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "wavelet-compression_amd" / "bin" / "wavelet-compression"
TOLS = (0.0, 1e-3, 1e-2, 0.1, 1.0, 100.0, math.inf)


def check(wc, counts, ncoeff, tol):
    got_t, got_b = wc.capi.tol_threshold(counts, ncoeff, tol)
    want_t, want_b = tol_rule(counts, ncoeff, tol)
    assert same_bits(got_t, want_t, np.float32), (tol, got_t, want_t)
    assert same_bits(got_b, want_b), (tol, got_b, want_b)
    assert got_b <= tol
    return got_t, got_b


def test_tol_threshold_matches_restatement(wc):
    rng = np.random.default_rng(3)
    cases = []
    for _ in range(6):  # sparse
        h = np.zeros(HIST_BINS, np.uint64)
        idx = rng.integers(0, HIST_BINS, 40)
        h[idx] = rng.integers(1, 10 ** 6, 40).astype(np.uint64)
        cases.append(h)
    for _ in range(3):  # dense over the finite range of ordinary data
        h = np.zeros(HIST_BINS, np.uint64)
        h[700:1100] = rng.integers(0, 5000, 400).astype(np.uint64)
        h[0] = 12345
        cases.append(h)
    cases.append(rng.integers(1, 50, HIST_BINS).astype(np.uint64))  # every bin, NaN-free ones included
    for h in cases:
        n = int(h.sum())
        for tol in TOLS + (1e-30, 1e-12, 3.7, 1e6, 1e30):
            check(wc, h, n, tol)


def test_tol_threshold_edges(wc):
    empty = np.zeros(HIST_BINS, np.uint64)
    for tol in TOLS:
        assert check(wc, empty, 0, tol) == (FLT_MAX, 0.0)     # N = 0: nothing to keep
        assert check(wc, empty, 64, tol) == (FLT_MAX, 0.0)    # every coefficient NaN: not counted
    h = np.zeros(HIST_BINS, np.uint64)
    h[0], h[0xFEF], h[0xFF0] = 5, 2, 1  # zeros / tiny denormals, the last finite bin, +-inf
    n = 8
    assert check(wc, h, n, 0.0) == (0.0, 0.0)                 # tol 0: every non-zero coefficient kept
    t, b = check(wc, h, n, 1.0)                               # bin 0 dropped, the rest kept
    assert same_bits(t, float(np.array([(0xFEF << 19) - 1], np.uint32).view(np.float32)[0]), np.float32)
    assert 0.0 < b < 1e-38
    t, b = check(wc, h, n, 1e150)                             # the last finite bin's edge is +inf: a finite budget keeps it
    assert same_bits(t, float(np.array([(0xFEF << 19) - 1], np.uint32).view(np.float32)[0]), np.float32)
    assert check(wc, h, n, math.inf) == (FLT_MAX, math.inf)   # tol inf: only +-inf survives the strict test
    only_inf = np.zeros(HIST_BINS, np.uint64)
    only_inf[0xFF0] = 3
    t, b = check(wc, only_inf, 3, 5.0)
    assert same_bits(t, float(np.array([(0xFF0 << 19) - 1], np.uint32).view(np.float32)[0]), np.float32) and b == 0.0
    one = np.zeros(HIST_BINS, np.uint64)
    one[1000] = 1
    # the budget is met exactly at a bin edge: t <= budget drops the bin
    hi = float(np.array([1001 << 19], np.uint32).view(np.float32)[0])
    tol = math.sqrt(8.0 * hi * hi)
    if (tol * tol) * 1.0 >= 8.0 * (hi * hi):
        assert check(wc, one, 1, tol)[0] == FLT_MAX
    assert check(wc, one, 1, tol * 0.999)[0] < hi


def test_tol_threshold_rejects_bad_tolerance(wc):
    h = np.ones(HIST_BINS, np.uint64)
    for bad in (math.nan, -1.0, -0.5e-300, -math.inf):
        with pytest.raises(wc.WaveletError) as ei:
            wc.capi.tol_threshold(h, HIST_BINS, bad)
        assert ei.value.code == wc.capi.WC_ERR_INVALID


@pytest.mark.parametrize("dims", [(2, 2, 2), (4, 2, 6), (16, 16, 24)])
def test_rule_end_to_end_on_the_oracle(wc, oracle, dims):
    """decompose -> bins -> wc_tol_threshold -> payload -> reconstruction: the
    actual RMSE is within tol * (1 + MARGIN); the margin covers the fp32
    rounding of the round trip, which is first confirmed for each input
    (keep-everything RMSE <= FLOOR)."""
    W, H, D = dims
    for kind in range(4):
        box = field(kind, W, H, D, seed=11 + kind)
        assert np.abs(box).max() <= 8.0
        flat = oracle.wavelet_decompose(box)
        floor = oracle.rmse(box, oracle.decompress_payload(oracle.compress_payload_thresh(box, -1.0)))
        assert floor <= FLOOR, (dims, kind, floor)
        counts = oracle.magnitude_hist(flat)
        for tol in (1e-3, 1e-2, 0.1, 1.0, 100.0):
            t, bound = check(wc, counts, flat.size, tol)
            payload = oracle.compress_payload_thresh(box, t)
            # the model: the dropped coefficients' energy is within the bound
            dropped = flat[~(np.abs(flat) > np.float32(t))].astype(np.float64)
            model = math.sqrt(8.0 * float(np.sum(dropped * dropped)) / flat.size)
            assert model <= bound * (1 + 1e-12) + 1e-300, (dims, kind, tol, model, bound)
            actual = oracle.rmse(box, oracle.decompress_payload(payload))
            assert actual <= tol * (1 + MARGIN), (dims, kind, tol, actual)


def run_cli(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("mode", ["-c", "-estimate"])
@pytest.mark.parametrize("bad,comps", [("rmse=abc", "temp"), ("rmse=-0.5", "temp"), ("rmse=nan", "temp"),
                                       ("rmse=0.1x", "temp"), ("rmse=0.1 0.2 0.3", "temp pressure"),
                                       ("rmse=0.1 0.2", "temp pressure density")])
def test_cli_rejects_bad_rmse(tmp_path, mode, bad, comps):
    """A bad `rmse=` is reported like a bad xzpreset ([error] Bad ...) and the run
    stops before it reads or writes anything."""
    data, out = tmp_path / "data", tmp_path / "out"
    data.mkdir()
    r = run_cli(f"datadir={data}/", "minfile=plt00010", "maxfile=plt00011", "minlevel=0", "maxlevel=0",
                f"components={comps}", "keep=0.999", f"compresseddir={out}/", bad, mode)
    assert "[error] Bad rmse" in r.stderr, r.stdout + r.stderr
    assert not out.exists()
