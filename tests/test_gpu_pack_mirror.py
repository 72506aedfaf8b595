"""GPU: compress_packed of the C++ mirror (include/wavelet_amd/codec_extras.h)
through tests/cpp/test_compress_packed.cpp: the .xz files it writes hold the
restatement's packed units (pack_rule.py) of the payloads compress() writes, under
the reference's file names; the mirror's decompress(), decompress_coarse() and
decompress_region() and the Python decompress() read them to the same cells, those
of the restatement's quantised payload."""
import lzma
import subprocess
from pathlib import Path

import numpy as np
import pytest

import coarse_ref as C
import levels_ref as R
import pack_rule as PR
from tol_rule import field

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tools" / "bin"


@pytest.mark.parametrize("dims,V", [((32, 16, 48), 3), ((12, 20, 8), 2), ((7, 5, 3), 4), ((64, 64, 64), 3)])
def test_compress_packed_files_and_cells(tmp_path, oracle, dims, V):
    from wavelet_compression_amd import codec
    W, H, D = dims
    keep = float(np.float32(0.999))
    boxes = [field(k, W, H, D, seed=40 + k) for k in (0, 2)]
    raw = tmp_path / "box.raw"
    raw.write_bytes(b"".join(b.tobytes() for b in boxes))
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([str(BIN / "test_compress_packed"), str(raw), str(W), str(H), str(D), "2", repr(keep), str(V),
                        str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for c, b in enumerate(boxes):
        std = oracle.compress_payload(b, keep)[0]
        f = out / f"compressed-wavelet-7-1-{c}-3.xz"
        assert lzma.decompress(f.read_bytes(), format=lzma.FORMAT_XZ) == PR.pack(std, V)
        assert int(r.stdout.split()[c]) == (len(std) - 20) // 8
        quant = PR.quantise(std, V)
        want = R.decode(quant)[0]
        assert (out / f"cells-{c}.raw").read_bytes() == want.tobytes()  # the mirror's decompress()
        assert codec.decompress(f).tobytes() == want.tobytes()
        if W % 2 == 0 and H % 2 == 0 and D % 2 == 0:
            cells = tmp_path / "coarse.raw"
            rc = subprocess.run([str(BIN / "test_coarse"), str(f), "1", str(cells)], capture_output=True, text=True,
                                timeout=120)
            assert rc.returncode == 0, rc.stdout + rc.stderr
            assert cells.read_bytes() == C.decode(quant, 1).tobytes()
            lo, hi = (2, 0, 2), (W - 1, H // 2, D - 1)
            rr = subprocess.run([str(BIN / "test_region"), str(f), *map(str, lo), *map(str, hi), "0", str(cells)],
                                capture_output=True, text=True, timeout=120)
            assert rr.returncode == 0, rr.stdout + rr.stderr
            assert cells.read_bytes() == np.ascontiguousarray(want[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]).tobytes()
    if V == 4:  # lossless: the cells of compress()'s own files
        for c, b in enumerate(boxes):
            assert (out / f"cells-{c}.raw").read_bytes() == oracle.decompress_payload(oracle.compress_payload(b, keep)[0]).tobytes()
