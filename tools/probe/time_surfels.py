"""Time gc_extract_lidar_surfels at the reference's configuration (grid 32 x 32 x 8, 32 occupants,
1,024 surfels, 512 features, 0.1 m voxels) for N = 8,192 points (GC_N_POINTS_CAP) and N = 65,536.
The points are the synthetic three-plane scene of tests/surfel_cases.py, scaled by sqrt(N / 8192) so
the point density per cell stays that of the test. Each timed sample is one call between two events
on the context's stream: the call's six launches and its 4-byte n_valid download, outputs already
allocated and zeroed; warm-up calls first, then the median of --iters samples.

Beside each time: the bytes the call must move at least (N x 40 B of points, timestamps and weights
read once, the written rows) and the rate that implies. The call is launch- and latency-bound at
these sizes, so the rate is far below the memory system's.

    python tools/probe/time_surfels.py [--iters 100] [--json OUT]
"""

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "fl-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from gcslam import _abi  # noqa: E402
from gcslam.measurement_batch import BATCH_ARRAYS  # noqa: E402
from gcslam.ops import SurfelExtractionConfig  # noqa: E402
import surfel_cases as SC  # noqa: E402


def time_extract(ctx, n, iters, warmup):
    cfg = SurfelExtractionConfig()
    pts, t, w = SC.scene(n, 0)
    scale = float(np.sqrt(n / 8192.0))
    pts = np.where(np.abs(pts) < 1e5, pts * scale, pts)
    dp, dt, dw = (_abi.DeviceArray.from_host(ctx, a) for a in (pts, t, w))
    n_total, L = cfg.n_feat + cfg.n_surfel, 3
    names = list(BATCH_ARRAYS)
    blk = _abi.alloc_many(ctx, [((n_total,) + (shp if k != "etas" else (L, 3)), BATCH_ARRAYS[k][2])
                                for k, (shp, _, _) in BATCH_ARRAYS.items()] + [((cfg.n_surfel,), np.int32)])
    blk[0]._base.zero()
    c_cfg = _abi.cfg("gc_surfel_cfg", cfg, n_lobes=L)
    nv = C.c_int32(0)

    def call():
        _abi.call("gc_extract_lidar_surfels", ctx.handle, n, dp.ptr, dt.ptr, dw.ptr, C.byref(c_cfg),
                  *[b.ptr for b in blk[:len(names)]], blk[-1].ptr, C.byref(nv), ctx=ctx)

    e0, e1 = _abi.Event(ctx), _abi.Event(ctx)
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(iters):
        e0.record()
        call()
        e1.record()
        ctx.sync()
        ms.append(e0.elapsed_ms(e1))
    ms.sort()
    med = statistics.median(ms)
    row_bytes = 8 * (9 + 3 + 3 * L + 1 + 1 + 3) + 4 + 4 + 1
    moved = n * 40 + int(nv.value) * row_bytes
    row = dict(N=n, n_valid=int(nv.value), scene_scale=scale, median_us=1e3 * med, p10_us=1e3 * ms[len(ms) // 10],
               p90_us=1e3 * ms[(9 * len(ms)) // 10], iters=iters, min_bytes=moved, GBps=moved / (med * 1e-3) / 1e9)
    print(json.dumps(row), flush=True)
    return row


def time_library_sort(ctx, n, iters, warmup):
    """The other route to the bucket: the library's stable radix sort (gc_sort.hip, eight 8-bit passes
    over the double keys) of (cell, point index) pairs. Timed alone, so it is a lower bound for that
    route, which also needs the keys as doubles before it and the run starts after it."""
    rng = np.random.default_rng(0)
    dk = _abi.DeviceArray.from_host(ctx, rng.integers(0, 8192, n).astype(np.float64))
    dv = _abi.DeviceArray.from_host(ctx, np.arange(n, dtype=np.uint32), np.uint32)
    dko, dvo = _abi.DeviceArray(ctx, n), _abi.DeviceArray(ctx, n, np.uint32)
    e0, e1 = _abi.Event(ctx), _abi.Event(ctx)
    ms = []
    for it in range(warmup + iters):
        e0.record()
        _abi.call("gc_test_radix_sort", ctx.handle, dk.ptr, dv.ptr, 1, n, 0, dko.ptr, dvo.ptr, ctx=ctx)
        e1.record()
        ctx.sync()
        if it >= warmup:
            ms.append(e0.elapsed_ms(e1))
    ms.sort()
    row = dict(N=n, library_radix_sort_pairs_us=1e3 * statistics.median(ms), p10_us=1e3 * ms[len(ms) // 10],
               p90_us=1e3 * ms[(9 * len(ms)) // 10], iters=iters)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = _abi.default_context()
    cfg = SurfelExtractionConfig()
    res = dict(config={k: v for k, v in cfg.__dict__.items()},
               rows=[time_extract(ctx, n, a.iters, a.warmup) for n in (8192, 65536)],
               sort_alternative=[time_library_sort(ctx, n, a.iters, a.warmup) for n in (8192, 65536)])
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
