"""The host side of the tolerance forms of the compressed-domain thinning and split
under ASan + UBSan, without a GPU: tests/cpp/test_thin_tol.cpp, a stand-alone
program (`make thintolsan`) that runs wc_thin_tol_unit / wc_split_tol_unit and the
host drivers wc_thin_tol_host / wc_split_tol_host over the CPU fake of the HIP
runtime, every buffer a heap block of exactly its documented size.  Nothing is
loaded into this process."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "wavelet-compression_amd" / "csrc"


def test_rule_and_host_drivers_under_sanitizer():
    subprocess.run(["make", "-s", "-C", str(CSRC), "thintolsan"], check=True, timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0:exitcode=66",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=66")
    r = subprocess.run([str(ROOT / "tools" / "bin" / "asan" / "test_thin_tol")], capture_output=True, text=True,
                       timeout=600, env=env)
    text = r.stdout + r.stderr
    assert "Sanitizer" not in text and "runtime error:" not in text, text[-4000:]
    assert r.returncode == 0 and " 0 failed" in r.stdout, text[-4000:]
    assert int(r.stdout.split()[0]) > 1000, r.stdout
