"""GPU: the upper layers of the progressive layers against the numpy restatement
(layers_rule.py) on three small boxes, one of them given as a packed unit:
codec.split_payloads (max_bytes=, ratio=, thresh=) / codec.merge_payloads and
split_budget / split_thresh / merge of the C++ mirror
(include/wavelet_amd/codec_extras.h) through tests/cpp/test_layers_mirror.cpp."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import layers_rule as LR
from test_gpu_thin_mirror import inputs, pairs_of

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tools" / "bin" / "test_layers_mirror"


@pytest.mark.parametrize("ratio", [3.0, 16.0, 1e6])
def test_split_and_merge_payloads_by_ratio_and_bytes(wc, ratio):
    from wavelet_compression_amd import codec
    std, given = inputs(wc)
    want = [LR.split_budget(p, pairs_of(ratio, p))[:2] for p in std]
    bases, rests = codec.split_payloads(given, ratio=ratio)
    assert list(zip(bases, rests)) == want
    assert bases == codec.thin_payloads(given, ratio=ratio)
    nbytes = [20 + 8 * pairs_of(ratio, p) for p in std]
    assert codec.split_payloads(given, max_bytes=nbytes) == (bases, rests)
    assert codec.merge_payloads(bases, rests) == codec.merge_payloads(rests, bases) == std
    # a stack of three layers, any order of the fold
    b2, r2 = codec.split_payloads(rests, ratio=ratio * 2)
    assert list(zip(b2, r2)) == [LR.split_budget(r, pairs_of(ratio * 2, r))[:2] for r in rests]
    assert codec.merge_payloads(bases, b2, r2) == codec.merge_payloads(r2, bases, b2) == std
    assert codec.merge_payloads(bases, b2) == [LR.merge(a, b) for a, b in zip(bases, b2)]


@pytest.mark.parametrize("thresh", [0.0, 0.01, np.inf])
def test_split_and_merge_payloads_by_threshold(wc, thresh):
    from wavelet_compression_amd import codec
    std, given = inputs(wc)
    want = [LR.split_thresh(p, [thresh] * 4)[:2] for p in std]
    bases, rests = codec.split_payloads(given, thresh=thresh)
    assert list(zip(bases, rests)) == want
    packed_rests = [wc.capi.pack_unit(r, 4) for r in rests]  # packed layers are unpacked first
    assert codec.merge_payloads(bases, packed_rests) == std
    for bad in (dict(), dict(ratio=2.0, thresh=0.1), dict(ratio=0.0), dict(max_bytes=19)):
        with pytest.raises(ValueError):
            codec.split_payloads(given, **bad)
    with pytest.raises(ValueError):
        codec.merge_payloads(bases, rests[:-1])
    if 0 < thresh < np.inf:  # the layers of one unit overlap with themselves
        with pytest.raises(wc.WaveletError) as ei:
            codec.merge_payloads(bases, bases)
        assert ei.value.code == wc.capi.WC_ERR_FORMAT
    assert codec.split_payloads([], thresh=thresh) == ([], []) and codec.merge_payloads([], []) == []


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
        want = [LR.split_budget(p, pairs_of(value, p))[:2] for p in std]
    else:
        want = [LR.split_thresh(p, [np.float32(value)] * 4)[:2] for p in std]
    n = len(std)
    assert got[:n] == [w[0] for w in want] and got[n:2 * n] == [w[1] for w in want]
    assert got[2 * n:] == std
