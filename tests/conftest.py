import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def pytest_collection_finish(session):
    # One HIP runtime per process: torch must come before libsgdnet_hip.so wherever sgdnet_amd.parallel is used
    # (sgdnet_amd/_lib.py).  The GPU fixtures import it first, but CPU tests load the library without it, so a session
    # that runs both would hand the GPU tests a library loaded before torch.  Sessions without GPU tests never import it.
    if any(item.get_closest_marker("gpu") for item in session.items):
        import torch  # noqa: F401


@pytest.fixture(scope="session")
def oracle():
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle
