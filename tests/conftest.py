import gc
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu)")


@pytest.fixture(scope="session")
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _collect_between_modules():
    gc.collect()                 # (dead cycles of the previous module's GPU tests go now, not at some later moment)
    yield


@pytest.fixture(autouse=True)
def _no_gc_inside_graph_captures(request):
    """GPU tests run with the automatic collector off; it runs again between tests.  torch no longer collects when a graph
    capture begins, so a dead reference cycle left by an earlier test (a captured step holding its graphs and their
    memory pool) could otherwise be collected in the middle of a capture, and its destructor would free device memory
    inside the capture -- which aborts the process."""
    if request.node.get_closest_marker("gpu") is None:
        yield
        return
    gc.disable()
    try:
        yield
    finally:
        gc.enable()


def pytest_sessionfinish(session, exitstatus):
    from tests import margins
    margins.dump(ROOT)


def pytest_terminal_summary(terminalreporter):
    from tests import margins
    if not margins.RECORDS:
        return
    terminalreporter.write_sep("-", "parity margins (measured / tolerance)")
    for r in margins.RECORDS:
        terminalreporter.write_line(f"{r['measured']:.3e} / {r['tolerance']:.1e} ({100 * r['used']:.0f} %)  {r['test']} {r['what']}")
