import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (runs the HIP path through the C ABI)")
    config.addinivalue_line("markers", "slow: long-running")


@pytest.fixture(scope="session")
def oracle():
    import oracle_py
    oracle_py.lib()
    return oracle_py


@pytest.fixture(scope="session")
def golden():
    import json

    import numpy as np
    # (two files: each committed fixture stays under 1 MiB)
    g = dict(np.load(os.path.join(TESTS, "golden", "clouds.npz")))
    g.update(np.load(os.path.join(TESTS, "golden", "clouds_vtk.npz")))
    with open(os.path.join(TESTS, "golden", "kat.json")) as f:
        kat = json.load(f)
    return g, kat
