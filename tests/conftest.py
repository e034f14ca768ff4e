import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


# The CPU oracle's fp32 results follow the thread count (MKL and ATen split their sums by it).  The GPU tests feed those results
# to the kernels as teacher-forced inputs, where a chain whose input moved by an ulp can cross a ReLU kink on one side and not
# the other, so a GPU test runs the oracle on one thread whatever OMP_NUM_THREADS says.  The CPU tests keep the process default
# (their bit-exact comparisons with the recorded fixtures hold on it, and not on one thread on every host).
_DEFAULT_THREADS = torch.get_num_threads()


@pytest.hookimpl(tryfirst=True)
def pytest_runtest_setup(item):
    torch.set_num_threads(1 if item.get_closest_marker("gpu") is not None else _DEFAULT_THREADS)


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN
