"""GPU: compress_maxerr of the C++ mirror (include/wavelet_amd/codec_extras.h)
through tests/cpp/test_compress_maxerr.cpp: the .xz files it writes hold the
restatement's payloads (maxerr_rule.py) at the levels each box admits, under
the reference's file names, and decompress through the Python codec within the
bound."""
import lzma
import subprocess
from pathlib import Path

import pytest

import levels_ref as R
import maxerr_rule as MR
from tol_rule import field

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tools" / "bin" / "test_compress_maxerr"


@pytest.mark.parametrize("dims,levels,bound", [((32, 16, 48), 4, 0.05), ((12, 20, 8), 3, 0.5), ((6, 10, 14), 2, 0.01)])
def test_compress_maxerr_writes_the_restatements_payloads(tmp_path, dims, levels, bound):
    from wavelet_compression_amd import codec
    W, H, D = dims
    boxes = [field(k, W, H, D, seed=20 + k) for k in (0, 2)]
    raw = tmp_path / "box.raw"
    raw.write_bytes(b"".join(b.tobytes() for b in boxes))
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([str(BIN), str(raw), str(W), str(H), str(D), "2", str(levels), repr(bound), str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    L = R.levels_for(W, H, D, levels)
    for c, b in enumerate(boxes):
        want, kept, _, err, bstar = MR.payload(b, L, bound)
        assert bstar > 0 and err <= bound
        f = out / f"compressed-wavelet-7-1-{c}-3.xz"
        assert lzma.decompress(f.read_bytes(), format=lzma.FORMAT_XZ) == want
        assert int(r.stdout.split()[c]) == kept
        regen = codec.decompress(f)
        assert regen.shape == b.shape and MR.max_abs(b, regen) == err
