import os
import sys

import pytest

# torch's CPU erfinv (trunc_normal_ initialisation) goes through MKL, whose default code path differs between Intel and AMD CPUs
# in the last bits; the bit-exact initialisation goldens (F12, F16) hold on both only in MKL's SSE2 path, which AMD CPUs always
# take.  Set before torch (and MKL) is loaded; tests/golden/make_golden.py pins the same path.
os.environ["MKL_CBWR"] = "COMPATIBLE"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vit-search_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def pytest_collection_modifyitems(config, items):
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU visible")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


@pytest.fixture(scope="session")
def golden_dir():
    return os.path.join(ROOT, "tests", "golden")


def pytest_sessionfinish(session, exitstatus):
    """Leave the GPU quiet before the interpreter tears down: captured graphs, side streams and workspaces are released while the HIP
    runtime is still alive (an abort inside the runtime's own exit handlers would turn a green run into a non-zero exit code)."""
    try:
        import gc
        import torch
        if torch.cuda.is_available():
            torch.cuda.synchronize()
            gc.collect()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
    except Exception:       # noqa: BLE001
        pass
