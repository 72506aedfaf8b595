"""GPU: compress_budget of the C++ mirror (include/wavelet_amd/codec_extras.h)
through tests/cpp/test_compress_budget.cpp: the .xz files it writes hold the
restatement's payloads (budget_rule.py) at the levels each box admits and at the
pair budget of the ratio, under the reference's file names, within the byte
bound; the Python codec gives the same bytes for max_bytes= and ratio=, and
decompress(coarsen=, region=) reads the files as they are."""
import lzma
import subprocess
from pathlib import Path

import numpy as np
import pytest

import budget_rule as BR
import coarse_ref as C
import levels_ref as R
from test_gpu_fuzz import same_cells
from tol_rule import field

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tools" / "bin" / "test_compress_budget"


@pytest.mark.parametrize("dims,levels,ratio", [((32, 16, 48), 4, 20.0), ((12, 20, 8), 3, 7.5), ((6, 10, 14), 2, 2.0),
                                               ((8, 8, 8), 3, 1e6)])
def test_compress_budget_writes_the_restatements_payloads(tmp_path, dims, levels, ratio):
    from wavelet_compression_amd import codec
    W, H, D = dims
    boxes = [field(k, W, H, D, seed=20 + k) for k in (0, 2)]
    raw = tmp_path / "box.raw"
    raw.write_bytes(b"".join(b.tobytes() for b in boxes))
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([str(BIN), str(raw), str(W), str(H), str(D), "2", str(levels), repr(ratio), str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    L = R.levels_for(W, H, D, levels)
    max_bytes = max(20, int(4 * W * H * D / ratio))
    K = (max_bytes - 20) // 8
    by_ratio = codec.compress_payloads(boxes, keep=0.5, levels=levels, ratio=ratio)
    by_bytes = codec.compress_payloads(boxes, keep=0.5, levels=levels, max_bytes=max_bytes)
    for c, b in enumerate(boxes):
        want, kept = BR.payload(b, L, K)[:2]
        assert kept <= K and len(want) <= max_bytes
        f = out / f"compressed-wavelet-7-1-{c}-3.xz"
        assert lzma.decompress(f.read_bytes(), format=lzma.FORMAT_XZ) == want
        assert int(r.stdout.split()[c]) == kept
        assert by_ratio[c] == want and by_bytes[c] == want
        full = R.decode(want)[0]
        assert same_cells(codec.decompress(f).ravel(), full.ravel())
        assert same_cells(codec.decompress(f, coarsen=1).ravel(), C.decode(want, 1).ravel())
        lo, hi = (1, 0, 2), (W - 1, H // 2, D - 1)
        got = codec.decompress(f, region=(lo, hi))
        crop = full[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
        assert got.shape == crop.shape and same_cells(got.ravel(), crop.ravel())
