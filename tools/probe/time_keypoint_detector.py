"""Time gc_keypoints_detect at the node's budget: a 640 x 480 rgb8 image, the default OrbDetectorConfig
(512 features, scale 1.2, 8 levels, edge 31, FAST threshold 20, Harris). The image is the colour image
of the detector's chain test (tests/keypoint_cases.py: random rectangles plus +-6 noise) at this size;
--images noise adds uniform noise, the densest input (the candidate list is sorted at its capacity
either way). Each timed sample is one call between two events on the context's stream: the image
resident, the pyramid and the outputs allocated, nothing downloaded. Warm-up calls first, then the
median of --iters samples with p10 and p90.

The launches and the bytes of a call are computed from the plan's shapes, not measured. Per-kernel times
come from running this probe on its own under `rocprofv3 --kernel-trace --stats` (no counters alongside).

    python tools/probe/time_keypoint_detector.py [--iters 20] [--warmup 3] [--images scene noise] [--json OUT]
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

W, H = 640, 480
SORT_PASSES = 5     # gc_keypoints.hip kKpSortPasses: the 38-bit keys take five 8-bit passes of three kernels


def _stats(ms):
    ms = sorted(ms)
    return dict(median_us=1e3 * statistics.median(ms), p10_us=1e3 * ms[len(ms) // 10],
                p90_us=1e3 * ms[(9 * len(ms)) // 10], iters=len(ms))


def shape_counts(plan, channels=3):
    """Launches (kernels, memsets and table uploads) and bytes of one call, from the shapes alone."""
    L = len(plan["sizes"])
    px = [w * h for w, h in plan["sizes"]]
    cap = sum(plan["caps"])
    slots = sum(min(2 * q, c) for q, c in zip(plan["quotas"], plan["caps"]))
    tabs = sum(8 * (w + h) for w, h in plan["sizes"][1:])
    sort_tiles = -(-cap // 2048)
    per_pass = 8 * cap * 3 + 4 * 256 * sort_tiles * 3     # keys read twice and written once, tile counts
    b = dict(image_read=channels * px[0], grey_write=px[0],
             resize=sum(4 * d + d for d in px[1:]) + tabs, table_upload=tabs,
             fast_read=sum(px), list_fill=8 * cap, sort=SORT_PASSES * per_pass,
             harris=slots * (81 + 8 + 8), select=slots * 16 + 3 * 8 * sum(plan["quotas"]) + 4 * 4 * sum(plan["quotas"]))
    launches = dict(memset=2, grey=1, table_upload=1 if tabs <= 512 << 10 else L - 1, resize=L - 1, fast=1,
                    sort=3 * SORT_PASSES, harris=1, select=1)
    return launches, b


def time_detect(ctx, name, image, iters, warmup):
    from gcslam import _abi
    from gcslam.ops import OrbDetectorConfig
    from gcslam.ops.keypoint_detector import _cfg, keypoints_plan
    cfg = OrbDetectorConfig()
    c_cfg = _cfg(cfg)
    plan = keypoints_plan(H, W, cfg)
    d_img = _abi.DeviceArray.from_host(ctx, image, np.uint8)
    d_pyr = _abi.DeviceArray(ctx, (plan["pyramid_bytes"],), np.uint8)
    k = cfg.max_features
    d_kp, d_meta, d_counts = _abi.alloc_many(ctx, [((k, 3), np.float64), ((k, 4), np.int32),
                                                   ((_abi.GC_KP_COUNTS_LEN,), np.int32)])

    def call():
        _abi.call("gc_keypoints_detect", ctx.handle, H, W, 3, d_img.ptr, C.byref(c_cfg), d_pyr.ptr, d_kp.ptr,
                  d_meta.ptr, d_counts.ptr, ctx=ctx)

    e0, e1 = _abi.Event(ctx), _abi.Event(ctx)
    for _ in range(warmup):
        call()
    ctx.sync()
    ms = []
    for _ in range(iters):
        e0.record()
        call()
        e1.record()
        ctx.sync()
        ms.append(e0.elapsed_ms(e1))
    c = d_counts.download()
    launches, b = shape_counts(plan)
    row = dict(what="gc_keypoints_detect", image=name, size=[W, H], **_stats(ms), keypoints=int(c[-1]),
               counts=c[:24].reshape(8, 3).tolist(), launches=launches, launches_total=sum(launches.values()),
               bytes=b, bytes_total=sum(b.values()), pyramid_bytes=plan["pyramid_bytes"],
               workspace_bytes=plan["workspace_bytes"], candidate_capacity=sum(plan["caps"]))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", nargs="+", default=["scene"], choices=["scene", "noise"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import keypoint_cases as KC
    from gcslam import _abi
    ctx = _abi.default_context()
    images = dict(scene=lambda: KC.scene(W, H, (500.0, 500.0, 320.0, 240.0))[1], noise=lambda: KC._noise(W, H))
    rows = [time_detect(ctx, name, images[name](), a.iters, a.warmup) for name in a.images]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(size=[W, H], rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
