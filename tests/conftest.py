import os
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

# Registers the package under its importable name `wavelet_compression_amd`
# (the directory name has a dash); loading it does not touch the GPU.
import wcamd  # noqa: E402,F401


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (HIP device)")


@pytest.fixture(scope="session")
def oracle():
    from oracle import oracle as O
    O.lib()
    return O


@pytest.fixture(scope="session")
def ref_tests(tmp_path_factory):
    """A directory holding the reference's fixtures plt00074 and plt00075,
    rebuilt in place of a checkout of the reference and verified against its
    recorded hashes before any test reads them."""
    from ref_plotfiles import check_ref_plotfiles, write_ref_plotfiles
    dst = tmp_path_factory.mktemp("ref_tests")
    write_ref_plotfiles(dst)
    check_ref_plotfiles(dst)
    return dst


@pytest.fixture(scope="session")
def wc():
    import wcamd
    wcamd.capi.load_library()
    return wcamd


@pytest.fixture(scope="session")
def ctx(wc):
    c = wc.capi.Context(0)
    yield c
    c.close()
