import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu)")


def load_gold(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


@pytest.fixture(scope="session")
def gold():
    return load_gold


# the goldens were made with this many intra-op CPU threads (tests/golden/make_goldens.py); CPU reductions round
# differently with the thread count, so the tests that reproduce them bit for bit pin it instead of taking the host's
GOLDEN_THREADS = 8


@pytest.fixture
def golden_threads():
    import torch
    before = torch.get_num_threads()
    torch.set_num_threads(GOLDEN_THREADS)
    yield GOLDEN_THREADS
    torch.set_num_threads(before)
