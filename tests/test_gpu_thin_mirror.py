"""GPU: the upper layers of the compressed-domain thinning against the numpy
restatement (thin_rule.py) on three small boxes, one of them given as a packed
unit: codec.thin_payloads (max_bytes=, ratio=, thresh=) and thin_budget /
thin_thresh of the C++ mirror (include/wavelet_amd/codec_extras.h) through
tests/cpp/test_thin_mirror.cpp."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import levels_ref as R
import pack_rule as PR
import thin_rule as TR
from tol_rule import field

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tools" / "bin" / "test_thin_mirror"
SPEC = [((16, 16, 16), 4, 0), ((12, 20, 8), 2, 2), ((6, 10, 14), 1, 1)]
PACKED = 1  # this one is handed over as a packed unit with 4 value bytes (lossless)
_memo = {}


def inputs(wc):
    """-> (standard thresh = 0 payloads, the list as handed over)."""
    if not _memo:
        std = [R.payload(field(k, *d, seed=70 + i), L, thresh=0.0)[0] for i, (d, L, k) in enumerate(SPEC)]
        given = list(std)
        given[PACKED] = wc.capi.pack_unit(std[PACKED], 4)
        assert PR.quantise(std[PACKED], 4) == std[PACKED]
        _memo["in"] = (std, given)
    return _memo["in"]


def pairs_of(ratio, pay):
    W, H, D = TR.parse(pay)[:3]
    return (max(20, int(4 * W * H * D / ratio)) - 20) // 8


@pytest.mark.parametrize("ratio", [3.0, 16.0, 1e6])
def test_thin_payloads_by_ratio_and_bytes(wc, ratio):
    from wavelet_compression_amd import codec
    std, given = inputs(wc)
    want = [TR.thin_budget(p, pairs_of(ratio, p))[0] for p in std]
    assert codec.thin_payloads(given, ratio=ratio) == want
    nbytes = [20 + 8 * pairs_of(ratio, p) for p in std]
    assert codec.thin_payloads(given, max_bytes=nbytes) == want
    assert all(len(w) <= b for w, b in zip(want, nbytes))
    assert codec.thin_payloads(want, ratio=ratio) == want  # idempotent


@pytest.mark.parametrize("thresh", [0.0, 0.01, np.inf])
def test_thin_payloads_by_threshold(wc, thresh):
    from wavelet_compression_amd import codec
    std, given = inputs(wc)
    want = [TR.thin_thresh(p, [thresh] * 4)[0] for p in std]
    assert codec.thin_payloads(given, thresh=thresh) == want
    assert want == [R.payload(field(k, *d, seed=70 + i), L, thresh=thresh)[0] for i, (d, L, k) in enumerate(SPEC)]
    for bad in (dict(), dict(ratio=2.0, thresh=0.1), dict(ratio=0.0), dict(max_bytes=19)):
        with pytest.raises(ValueError):
            codec.thin_payloads(given, **bad)


@pytest.mark.parametrize("mode,value", [("ratio", 5.0), ("thresh", 0.02)])
def test_cpp_mirror(wc, tmp_path, mode, value):
    std, given = inputs(wc)
    files = []
    for i, p in enumerate(given):
        f = tmp_path / f"in{i}.bin"
        f.write_bytes(p)
        files.append(str(f))
    out = tmp_path / "out.bin"
    r = subprocess.run([str(BIN), mode, repr(value), str(out)] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    blob, got = out.read_bytes(), []
    while blob:
        n = int(np.frombuffer(blob[:8], "<u8")[0])
        got.append(blob[8:8 + n])
        blob = blob[8 + n:]
    if mode == "ratio":
        want = [TR.thin_budget(p, pairs_of(value, p))[0] for p in std]
    else:
        want = [TR.thin_thresh(p, [np.float32(value)] * 4)[0] for p in std]
    assert got == want
