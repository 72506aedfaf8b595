"""GPU: the callers that read packed files (the C++ mirror's decompress() and
decompress_coarse() and the command line's -d through the direct decoders,
decompress_region() still through wc_unpack_host) give the bits the unpack path
gave: codec.unpack_payloads followed by the standard calls, and for -d the
plotfile of the restatement's quantised payloads (the expectation
tests/test_cli_pack.py records for a pack=3 run).  A directory that mixes
packed and standard files decodes in two calls."""
import lzma
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import levels_ref as LR
import pack_rule as PR
from test_cli_pack import COMPS, GEOM, IDX, LEVELS, TIME, cli, packed3, plain, read, run, same_tree  # noqa: F401 (fixtures)
from tol_rule import field

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "tools" / "bin"


@pytest.mark.parametrize("dims,V", [((32, 16, 48), 3), ((16, 16, 16), 2), ((8, 24, 8), 4)])
def test_mirror_reads_packed_files_as_the_unpack_path_did(tmp_path, dims, V):
    from wavelet_compression_amd import codec
    W, H, D = dims
    keep = float(np.float32(0.999))
    boxes = [field(k, W, H, D, seed=60 + k) for k in (0, 1)]
    raw = tmp_path / "box.raw"
    raw.write_bytes(b"".join(b.tobytes() for b in boxes))
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([str(BIN / "test_compress_packed"), str(raw), str(W), str(H), str(D), "2", repr(keep), str(V),
                        str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lo, hi = (2, 0, 2), (W - 1, H // 2, D - 1)
    for c in range(2):
        f = out / f"compressed-wavelet-7-1-{c}-3.xz"
        packed = lzma.decompress(f.read_bytes(), format=lzma.FORMAT_XZ)
        assert codec.capi.payload_packed(packed) == (1, V)
        std = codec.unpack_payloads([packed])  # the unpack path: standard payloads, then the standard calls
        assert codec.capi.payload_packed(std[0])[1] == 0
        want = codec.decompress_payloads(std)[0]
        assert (out / f"cells-{c}.raw").read_bytes() == want.tobytes()  # the mirror's decompress()
        cells = tmp_path / "cells.raw"
        rc = subprocess.run([str(BIN / "test_coarse"), str(f), "1", str(cells)], capture_output=True, text=True, timeout=120)
        assert rc.returncode == 0, rc.stdout + rc.stderr
        assert cells.read_bytes() == codec.decompress_payloads(std, coarsen=1)[0].tobytes()
        rr = subprocess.run([str(BIN / "test_region"), str(f), *map(str, lo), *map(str, hi), "0", str(cells)],
                            capture_output=True, text=True, timeout=120)
        assert rr.returncode == 0, rr.stdout + rr.stderr
        assert cells.read_bytes() == codec.decompress_payloads(std, region=(lo, hi))[0].tobytes()


def test_cli_d_of_packed_and_of_mixed_directories(run, plain, packed3, tmp_path):
    """-d of a pack=3 directory, and of one whose level-1 files are the standard ones of the run without pack=:
    the plotfiles written from the restatement's cells (quantised where the file is packed)."""
    from wavelet_compression_amd import plotfile as pf
    base = run[0]
    mixed = base / "mixedthree"
    shutil.copytree(packed3, mixed)
    for comp in IDX:
        shutil.copyfile(plain / f"compressed-wavelet-0-1-{comp}-0.xz", mixed / f"compressed-wavelet-0-1-{comp}-0.xz")
    for name, src, std_levels in (("three", packed3, ()), ("mixed", mixed, (1,))):
        cli(f"compresseddir={src}/", f"out={base}/direct{name}/", "-d")
        levels = []
        for l, boxes in enumerate(LEVELS):
            fabs = []
            for b, (lo, _) in enumerate(boxes):
                recon = []
                for comp in IDX:
                    std = read(plain, l, comp, b)
                    assert read(src, l, comp, b) == (std if l in std_levels else PR.pack(std, 3))
                    recon.append(LR.decode(std if l in std_levels else PR.quantise(std, 3))[0])
                fabs.append((lo, np.stack(recon).astype(np.float64)))
            levels.append(fabs)
        pf.write_plotfile(tmp_path / name / "plt00010", COMPS, TIME, GEOM, 2, (64, 32, 32), [100, 200], levels)
        same_tree(tmp_path / name / "plt00010", base / f"direct{name}" / "plt00010")
