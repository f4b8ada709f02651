import os
import sys

import pytest

# MKL serves torch's CPU erfinv / log / exp / erf with a code path chosen per processor, and the paths differ in the last bits
# (AVX-512 on Intel, a generic one on AMD).  Seeded initialisation goes through erfinv, and the goldens pin the reference's
# parameters bit for bit: the conditional-numerical-reproducibility mode COMPATIBLE is the same path on every x86 processor, and
# the goldens are generated under it.  Read by MKL at its first call, so it is set before any test module computes.
os.environ["MKL_CBWR"] = "COMPATIBLE"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu)")


def pytest_collection_modifyitems(config, items):
    import torch

    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN
