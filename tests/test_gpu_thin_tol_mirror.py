"""GPU: the upper layers of the tolerance forms of the compressed-domain thinning and
split against the numpy restatement (thin_tol_rule.py) on three small boxes, one of
them given as a packed unit: codec.thin_payloads(rmse=) / codec.split_payloads(rmse=)
and thin_rmse / split_rmse of the C++ mirror (include/wavelet_amd/codec_extras.h)
through tests/cpp/test_thin_tol_mirror.cpp."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import leveltol_rule as LT
import levels_ref as R
import pack_rule as PR
import thin_tol_rule as TT
from tol_rule import field

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tools" / "bin" / "test_thin_tol_mirror"
SPEC = [((16, 16, 16), 4, 0), ((12, 20, 8), 2, 2), ((6, 10, 14), 1, 1)]
PACKED = 1  # this one is handed over as a packed unit with 4 value bytes (lossless)
_memo = {}


def inputs(wc):
    """-> (boxes, standard thresh = 0 payloads, the list as handed over)."""
    if not _memo:
        boxes = [field(k, *d, seed=70 + i).astype(np.float32) for i, (d, L, k) in enumerate(SPEC)]
        std = [R.payload(b, L, thresh=0.0)[0] for b, (_, L, _) in zip(boxes, SPEC)]
        given = list(std)
        given[PACKED] = wc.capi.pack_unit(std[PACKED], 4)
        assert PR.quantise(std[PACKED], 4) == std[PACKED]
        _memo["in"] = (boxes, std, given)
    return _memo["in"]


@pytest.mark.parametrize("rmse", [0.0, 0.02, [0.5, 0.001, 0.1], math.inf])
def test_thin_and_split_payloads_by_rmse(wc, rmse):
    from wavelet_compression_amd import codec
    boxes, std, given = inputs(wc)
    tol = [rmse] * len(std) if np.ndim(rmse) == 0 else rmse
    want = [TT.thin_tol(p, t)[0] for p, t in zip(std, tol)]
    assert codec.thin_payloads(given, rmse=rmse) == want
    # the thresh = 0 payloads hold every candidate: the bytes of the forward at that tolerance
    assert want == [LT.payload(b, L, t)[0] for b, (_, L, _), t in zip(boxes, SPEC, tol)]
    assert want == codec.compress_payloads(boxes, 0.0, levels=4, rmse=rmse)
    bases, rests = codec.split_payloads(given, rmse=rmse)
    assert bases == want and rests == [TT.split_tol(p, t)[1] for p, t in zip(std, tol)]
    assert codec.merge_payloads(bases, rests) == std
    if rmse == 0.0:
        assert want == std
    if rmse == math.inf:
        assert all(len(w) == 20 for w in want)


def test_the_argument_forms(wc):
    from wavelet_compression_amd import codec
    _, std, given = inputs(wc)
    for call in (codec.thin_payloads, codec.split_payloads):
        for bad in (dict(), dict(rmse=0.1, thresh=0.1), dict(rmse=0.1, ratio=2.0), dict(rmse=0.1, max_bytes=100),
                    dict(rmse=-1.0), dict(rmse=math.nan), dict(rmse=[0.1, 0.2])):
            with pytest.raises(ValueError):
                call(given, **bad)
        with pytest.raises(ValueError):
            call([], rmse=0.1, thresh=0.2)
    assert codec.thin_payloads([], rmse=0.1) == [] and codec.split_payloads([], rmse=0.1) == ([], [])
    # existing call forms: positional max_bytes / ratio / thresh, device as a keyword
    assert codec.thin_payloads(given, None, None, 0.0) == std
    assert codec.thin_payloads(given, thresh=0.0, device=0) == std


@pytest.mark.parametrize("mode", ["thin", "split"])
def test_cpp_mirror(wc, tmp_path, mode):
    _, std, given = inputs(wc)
    rmse = 0.03
    files = []
    for i, p in enumerate(given):
        f = tmp_path / f"in{i}.bin"
        f.write_bytes(p)
        files.append(str(f))
    out = tmp_path / "out.bin"
    r = subprocess.run([str(BIN), mode, repr(rmse), str(out)] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    blob, got = out.read_bytes(), []
    while blob:
        n = int(np.frombuffer(blob[:8], "<u8")[0])
        got.append(blob[8:8 + n])
        blob = blob[8 + n:]
    want = [TT.thin_tol(p, rmse)[0] for p in std]
    if mode == "split":
        want = want + [TT.split_tol(p, rmse)[1] for p in std] + std
    assert got == want
    assert any(20 < len(w) < len(p) for w, p in zip(want, std))  # the tolerance bites, and not everything goes
