"""Multi-level mode without a GPU (include/wavelet_amd.h, "Opt-in multi-level
transform"): the host-only helpers wc_levels_for and wc_payload_levels; model
properties of the CPU restatement (levels_ref.py) that pin what the format
means; the CLI's `levels=` parameter checks."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import levels_ref as R

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "wavelet-compression_amd" / "bin" / "wavelet-compression"


def test_levels_for_table(wc):
    table = [((64, 64, 64), 4, 4), ((64, 64, 64), 2, 2), ((64, 64, 64), 1, 1), ((12, 20, 8), 3, 2),
             ((6, 8, 8), 2, 1), ((16, 8, 24), 3, 3), ((16, 8, 24), 4, 3), ((0, 8, 8), 3, 1), ((8, 8, 0), 4, 1),
             ((64, 64, 64), 9, 4), ((256, 256, 256), 9, 4), ((5, 7, 3), 4, 1), ((8, 8, 8), 0, 1), ((8, 8, 8), -3, 1)]
    for dims, want, L in table:
        assert wc.capi.levels_for(*dims, want) == L, (dims, want)
        assert R.levels_for(*dims, want) == L, (dims, want)
    assert wc.capi.WC_MAX_LEVELS == R.MAX_LEVELS == 4


def header(W, H, D, ncoeff, nrle=0):
    return np.array([W, H, D, ncoeff, nrle], "<i4").tobytes()


def test_payload_levels(wc):
    W, H, D = 16, 8, 24
    assert wc.capi.payload_levels(header(W, H, D, W * H * D)) == 1
    assert wc.capi.payload_levels(header(W, H, D, -2)) == 2
    assert wc.capi.payload_levels(header(W, H, D, -3, 77)) == 3
    assert wc.capi.payload_levels(header(64, 64, 64, -4)) == 4
    assert wc.capi.payload_levels(header(0, 4, 4, 0)) == 1
    # a bad ncoeff, and levels the dims do not admit
    for bad in (header(W, H, D, -5), header(W, H, D, 0), header(W, H, D, W * H * D + 1), header(W, H, D, -1),
                header(W, H, D, -4), header(6, 8, 8, -2), header(-16, 8, 24, -2)):
        with pytest.raises(wc.WaveletError) as ei:
            wc.capi.payload_levels(bad)
        assert ei.value.code == wc.capi.WC_ERR_FORMAT, np.frombuffer(bad, "<i4")
    with pytest.raises(wc.WaveletError) as ei:
        wc.capi.payload_levels(header(W, H, D, -2)[:19])
    assert ei.value.code == wc.capi.WC_ERR_INVALID


def synth(oracle, W, H, D):
    return oracle.narrow(oracle.synth_box_f64(oracle.unit_seed(0, 0, 3, 1), (0, 0, 0), W, H, D))


@pytest.mark.parametrize("dims", [(32, 32, 32), (16, 8, 24)])
def test_model_properties_of_the_restatement(oracle, dims):
    """More levels keep fewer coefficients at the same keep; with an explicit
    threshold t every cell is within (7 L + 1) t of the original, plus the
    restatement's own rounding e0 (its max error on this box with everything
    kept, t = -1): a cell is a +-1 sum of 7 details per level and one low-pass
    value, each dropped one at most t."""
    box = synth(oracle, *dims)
    kept = [R.payload(box, L, keep=0.99)[1] for L in (1, 2, 3)]
    print(dims, "kept at keep 0.99:", kept)
    assert kept[2] < kept[1] < kept[0]
    assert kept[0] == box.size // 8  # exactly the low-pass octant: the floor that further levels remove
    for L in (1, 2, 3):
        full, n = R.payload(box, L, thresh=-1.0)
        assert n == box.size
        regen, got = R.decode(full)
        assert got == L
        e0 = float(np.max(np.abs(regen.astype(np.float64) - box)))
        for t in (0.25, 2.0, 20.0):
            p, n = R.payload(box, L, thresh=t)
            regen, got = R.decode(p)
            err = float(np.max(np.abs(regen.astype(np.float64) - box)))
            print(dims, L, t, "kept", n, "max err", err, "bound", (7 * L + 1) * t + e0)
            assert got == L and err <= (7 * L + 1) * t + e0, (dims, L, t, err, e0)


def test_level_one_is_the_reference_payload(oracle):
    """L = 1 of the restatement is the oracle's compress_payload, header included;
    L >= 2 differs from it only as defined (ncoeff = -L, the corner transformed)."""
    box = synth(oracle, 16, 8, 24)
    assert R.payload(box, 1, keep=0.999) == oracle.compress_payload(box, 0.999)
    p2, _ = R.payload(box, 2, thresh=-1.0)
    (W, H, D), nc, runs, vals = oracle.parse_payload(p2)
    assert (W, H, D, nc) == (16, 8, 24, -2)
    one = oracle.wavelet_decompose(box).reshape(W, H, D)
    two = R.decompose(box, 2).reshape(W, H, D)
    outside = np.ones((W, H, D), bool)
    outside[:W // 2, :H // 2, :D // 2] = False
    assert np.array_equal(one[outside], two[outside])  # level-1 details are untouched
    assert not np.array_equal(one[~outside], two[~outside])


def run_cli(*args):
    return subprocess.run([str(CLI), *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("mode", ["-c", "-estimate"])
@pytest.mark.parametrize("bad,expect", [("levels=0", "Bad levels"), ("levels=5", "Bad levels"),
                                        ("levels=two", "Bad levels"), ("levels=2x", "Bad levels"),
                                        ("levels=-1", "Bad levels"), ("levels=2 3", "Bad levels"),
                                        ("levels=2.5", "Bad levels"),
                                        ("levels=2 rmse=0.1", "levels= cannot be combined with rmse=")])
def test_cli_rejects_bad_levels(tmp_path, mode, bad, expect):
    """A bad `levels=`, or `levels=` with `rmse=`, is reported like a bad rmse=
    and the run stops before it reads or writes anything."""
    data, out = tmp_path / "data", tmp_path / "out"
    data.mkdir()
    r = run_cli(f"datadir={data}/", "minfile=plt00010", "maxfile=plt00011", "minlevel=0", "maxlevel=0",
                "components=temp", "keep=0.999", f"compresseddir={out}/", *bad.split(" ", 1), mode)
    assert "[error] " + expect in r.stderr, r.stdout + r.stderr
    assert not out.exists()
