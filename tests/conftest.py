import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kotoba-whisper_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLD = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (runs on the GPU box via gpurun)")
    config.addinivalue_line("markers", "slow: minutes of CPU time")


def pytest_collection_modifyitems(config, items):
    """``slow`` tests (the numpy oracle's large-v3 / kotoba-v2 / long-form pins: minutes of single-threaded
    numpy each) run when selected explicitly (``-m slow``) or with KW_SLOW=1, so the default CPU suite stays
    within a few minutes.  Their last full run is recorded in profiles/README.md."""
    if os.environ.get("KW_SLOW") or "slow" in (config.getoption("markexpr") or "").replace("not slow", ""):
        return
    skip = pytest.mark.skip(reason="slow oracle pin: run with -m slow or KW_SLOW=1")
    for it in items:
        if "slow" in it.keywords:
            it.add_marker(skip)


def gpu_available() -> bool:
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="session")
def gold():
    from oracle.fixtures import load_fixture

    cache = {}

    def load(name):
        if name not in cache:
            path = os.path.join(GOLD, name + ".npz")
            if not os.path.exists(path):
                pytest.skip(f"golden fixture {name} not generated")
            cache[name] = load_fixture(path)  # with the arrays kept as row blocks in <name>.part<k>.npz
        return cache[name]

    return load
