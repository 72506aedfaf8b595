"""GPU: compress_rmse of the C++ mirror (include/wavelet_amd/codec_extras.h)
through tests/cpp/test_compress_rmse.cpp: the .xz files it writes hold the
restatement's payloads (leveltol_rule.py) at the levels each box admits, under
the reference's file names, and decompress through the Python codec within the
tolerance."""
import lzma
import subprocess
from pathlib import Path

import numpy as np
import pytest

import leveltol_rule as LT
import levels_ref as R
from tol_rule import MARGIN, field

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tools" / "bin" / "test_compress_rmse"


@pytest.mark.parametrize("dims,levels,tol", [((32, 16, 48), 4, 0.05), ((12, 20, 8), 3, 0.5), ((6, 10, 14), 2, 0.01)])
def test_compress_rmse_writes_the_restatements_payloads(oracle, tmp_path, dims, levels, tol):
    from wavelet_compression_amd import codec
    W, H, D = dims
    boxes = [field(k, W, H, D, seed=20 + k) for k in (0, 2)]
    raw = tmp_path / "box.raw"
    raw.write_bytes(b"".join(b.tobytes() for b in boxes))
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([str(BIN), str(raw), str(W), str(H), str(D), "2", str(levels), repr(tol), str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    L = R.levels_for(W, H, D, levels)
    for c, b in enumerate(boxes):
        want, kept = LT.payload(b, L, tol)[:2]
        f = out / f"compressed-wavelet-7-1-{c}-3.xz"
        assert lzma.decompress(f.read_bytes(), format=lzma.FORMAT_XZ) == want
        assert int(r.stdout.split()[c]) == kept
        regen = codec.decompress(f)
        assert regen.shape == b.shape and oracle.rmse(b, regen) <= tol * (1 + MARGIN)
