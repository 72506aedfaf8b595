"""wc_maxerrrule.cpp alone in the stand-alone program tests/cpp/test_maxerr.cpp,
built once plain (`make maxerrtest`) and once with ASan + UBSan (`make
maxerrsan`), on a table from the numpy restatement (maxerr_rule.py): exactly
W*H*D coefficients and W*H*D cells per case on the heap, so a read or write past
either is reported.  Nothing is loaded into this process."""
import os
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import levels_ref as R
import maxerr_rule as MR
from test_maxerr_cpu import bounds, units

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "wavelet-compression_amd" / "csrc"


def _bits64(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    lines = []
    for name, x, L in units():
        if x.size > 4096:
            continue
        D, H, W = x.shape
        flat = R.decompose(x.astype(np.float32), L)
        body = " ".join(f"{int(v):x}" for v in flat.view(np.uint32))
        cells = " ".join(f"{int(v):x}" for v in x.ravel().view(np.uint32 if x.dtype == np.float32 else np.uint64))
        for E in bounds(x):
            t, e, b = MR.select(x, L, E)
            tb = int(np.array([t], np.float32).view(np.uint32)[0])
            lines.append(f"{W} {H} {D} {L} {1 if x.dtype == np.float64 else 0} {_bits64(E):x} {b} {tb:x} "
                         f"{_bits64(e):x} {body} {cells}")
    path = tmp_path_factory.mktemp("maxerr") / "maxerr_table.txt"
    path.write_text("\n".join(lines) + "\n")
    return path, len(lines)


@pytest.mark.parametrize("target,binary", [("maxerrtest", "tools/bin/test_maxerr"),
                                           ("maxerrsan", "tools/bin/asan/test_maxerr")])
def test_host_rule_program(table, target, binary):
    path, cases = table
    subprocess.run(["make", "-s", "-C", str(CSRC), target], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0:exitcode=66",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=66")
    r = subprocess.run([str(ROOT / binary), str(path)], capture_output=True, text=True, timeout=600, env=env)
    text = r.stdout + r.stderr
    assert "Sanitizer" not in text and "runtime error:" not in text, text[-4000:]
    assert r.returncode == 0 and f"{cases} cases" in r.stdout and " 0 failed" in r.stdout, text[-4000:]
