import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "sixteen_processes: puts up to sixteen processes of its own on the GPU (eight ranks, each with its "
                                       "peer-to-peer probe child); runs before any test opens the GPU in the pytest process itself")


def _gpu_visible() -> bool:
    """Asked in a child process: torch.cuda.is_available() opens a device context, which would stay open in the pytest process for the
    whole session -- next to the sixteen of the eight-rank rehearsal below (eight bench.py ranks, each with its peer-to-peer probe child)."""
    import subprocess
    code = "import sys, torch; sys.exit(0 if torch.cuda.is_available() else 1)"
    return subprocess.run([sys.executable, "-c", code], capture_output=True).returncode == 0


def pytest_collection_modifyitems(config, items):
    """GPU tests are skipped (not failed) when no device is visible, e.g. `pytest tests/` here.  The bench rehearsals run FIRST: they put up to
    eight bench.py ranks on the one GPU, whose exchange kernels wait for each other on the device -- with the pytest process itself holding a
    ninth GPU context (any in-process GPU test before them) the driver time-slices whole processes and the ranks' bounded waits run out
    (5 of 7 in-suite runs failed that way on the round-5 boxes, 0 of 5 with the rehearsals first or alone)."""
    runs_first = lambda it: it.fspath.basename == "test_bench_gpu.py" or it.get_closest_marker("sixteen_processes") is not None  # noqa: E731
    first = [it for it in items if runs_first(it)]
    if first:
        items[:] = first + [it for it in items if not runs_first(it)]
    if _gpu_visible():
        return
    skip = pytest.mark.skip(reason="no GPU visible")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN
