"""The task plan of the persistent bins launch (gc_bins_task_plan, host-only: gc_binplan.h's plan_bins_tasks,
the arithmetic scan_bins_pipeline runs): the three chunk tiers tile a scan's 256-point units exactly, every
chunk is non-empty, the tier lengths and the kernel form follow the long-task length, and recorded rows of the
plan stay as they are (the plan fixes the order of summation, so a changed row changes output bits)."""

import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fl-slam_amd", "gcslam", "libgcslam.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libgcslam.so not built")

HS = [1, 2, 3, 4, 8, 32, 64, 128, 256, 1024]
CUS = [1, 8, 32, 64, 256, 304]
NCAPS = [1, 255, 256, 257, 512, 1000, 4096, 8192, 65536, 65537, 200000, 2 ** 20]

# H_geom, n_cap, cu_count -> iters, iters_short, iters_tiny, k1, k2, chunks, ahead
ROWS = [
    ((256, 65536, 256), (32, 16, 4, 5, 5, 14, 0)),
    ((128, 65536, 256), (32, 16, 4, 4, 7, 15, 0)),
    ((64, 65536, 256), (16, 8, 2, 11, 8, 27, 1)),
    ((32, 65536, 256), (8, 4, 1, 22, 16, 54, 1)),
    ((1024, 65536, 256), (32, 16, 4, 6, 3, 13, 0)),
    ((4, 8192, 256), (2, 2, 1, 0, 0, 32, 1)),
    ((1, 1, 256), (2, 2, 1, 0, 0, 1, 1)),
    ((2, 257, 256), (2, 2, 1, 0, 0, 2, 1)),
    ((32, 65536, 304), (4, 2, 1, 49, 20, 89, 1)),
    ((8, 200000, 64), (16, 8, 2, 38, 17, 74, 1)),
]


def plan(H, n_cap, cus):
    from gcslam import _abi
    out = np.zeros(8, np.int64)
    _abi.call("gc_bins_task_plan", H, n_cap, cus, out.ctypes.data)
    return [int(v) for v in out]


@pytest.mark.parametrize("cus", CUS)
def test_plan_invariants(cus):
    for H, n_cap in itertools.product(HS, NCAPS):
        iters, it_s, it_t, k1, k2, chunks, ahead, pullers = plan(H, n_cap, cus)
        case = (H, n_cap, cus)
        U = -(-n_cap // 256)
        Ut = U - k1 * iters - k2 * it_s
        assert k1 >= 0 and k2 >= 0 and Ut >= 0, case
        n_tiny = -(-Ut // it_t)
        assert chunks == k1 + k2 + n_tiny, case
        assert iters in (2, 4, 8, 16, 32), case
        assert it_s == max(2, iters // 2) and it_t == max(1, it_s // 4), case
        assert ahead == (1 if iters < 32 else 0) and pullers == 2 * cus, case
        if n_tiny:
            assert (n_tiny - 1) * it_t < Ut, case  # the last tiny chunk holds points
        assert chunks >= 1 and H * chunks < 2 ** 32, case


@pytest.mark.parametrize("args,want", ROWS)
def test_plan_rows(args, want):
    assert tuple(plan(*args)[:7]) == want


def test_plan_argument_errors():
    from gcslam import _abi
    out = np.zeros(8, np.int64)
    for H, n_cap, cus in [(0, 65536, 256), (32, 0, 256), (32, 65536, 0)]:
        with pytest.raises(ValueError):
            _abi.call("gc_bins_task_plan", H, n_cap, cus, out.ctypes.data)
    with pytest.raises(ValueError):
        _abi.call("gc_bins_task_plan", 32, 65536, 256, None)
