import os
import sys

import pytest

# the oracle tests hold the torch-CPU oracle to fixtures of the reference at 1e-6; MKL's GEMM kernels round differently by CPU
# vendor and instruction set (an AMD host misses fixtures made on an Intel one by ~2e-6), so the fixtures (tools/make_golden*.py)
# and the suite both use MKL's vendor-independent COMPATIBLE branch.  Read at MKL's first call: before any test computes.
os.environ["MKL_CBWR"] = "COMPATIBLE"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    # the CPU oracle's torch ops within the CPUs this process owns: torch's default of one OpenMP thread per VISIBLE CPU (128 on
    # the GPU boxes, 16 CPUs' worth of quota) gets the whole process throttled by the container's CFS quota (puflow_amd/_host.py)
    from puflow_amd._host import limit_host_threads
    limit_host_threads()


@pytest.fixture(scope="session")
def golden_dir():
    return os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="session")
def pretrained_pu1k(golden_dir):
    """tests/golden/pretrained_pu1k.npz (the reference's trained checkpoint, its inputs and outputs) with the outputs as captured
    under the MKL branch pinned above: pretrained_pu1k_compat.npz holds their exact float32 differences to the file's own
    (tools/make_golden_pretrained.py).  A dict of arrays."""
    import numpy as np
    g = np.load(os.path.join(golden_dir, "pretrained_pu1k.npz"))
    d = np.load(os.path.join(golden_dir, "pretrained_pu1k_compat.npz"))
    out = {k: g[k] for k in g.files}
    for k in d.files:
        out[k] = out[k] + d[k]
    return out
