import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# The dispatch-path assertions of the GPU tests are written for the library's default pool of two dispatch queues per device
# (include/ssd.h, "the queue rule").  A runner that exports GPU_MAX_HW_QUEUES -- even the HIP runtime's own default, 4 -- would
# shrink that pool to one queue and send every 2-chain rollout through hipLaunchKernel.  Pin the pool before any test loads the
# library; the tests of the rule itself set both variables in their child processes.
os.environ.setdefault("SSD_AQL_QUEUES", "2")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "reference: needs /root/reference (build container only)")


def pytest_collection_modifyitems(config, items):
    have_ref = os.path.isdir("/root/reference/social_dilemmas")
    skip_ref = pytest.mark.skip(reason="/root/reference not present (GPU box)")
    for item in items:
        if "reference" in item.keywords and not have_ref:
            item.add_marker(skip_ref)
