"""Time gc_camera_features_lift at the node's budget: a 640 x 480 image (fx = fy = 500), M = 512
keypoints, the default VisualFeatureConfig (median3, 5 x 5 fit) and the hex sample. The depth is the
scene of tests/camfeat_cases.py at this image size (a 4 m wall with a bump, a slanted wall, a floor
and a far wall, 0.4 % noise, 6 % of the pixels without a depth); keypoints uniform over the image.
Each timed sample is one call between two events on the context's stream: one launch, images and
keypoints resident, outputs allocated. Warm-up calls first, then the median of --iters samples with
p10 and p90.

The upload of the two images (1.2 MB of float32 depth, 0.9 MB of rgb8) from pageable host memory to
HBM is timed separately, one gc_buffer_upload each, event to event and by the host's clock around
the call and the wait.

The call reads at least 9-25 depth pixels for the sample and 25 for the fit per keypoint (about
200 B), 3 B of colour and 24 B of keypoint, and writes 242 B: 0.24 MB at M = 512. It is one launch
of M single-wave workgroups and is bound by its latency, not by bytes.

    python tools/probe/time_camera_features.py [--iters 20] [--warmup 3] [--json OUT]
"""

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "fl-slam_amd"))

W, H, FX, FY, CX, CY = 640, 480, 500.0, 500.0, 320.0, 240.0
M = 512


def scene(seed=0):
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dx, dy = (u - CX) / FX, (v - CY) / FY
    z = np.full((H, W), 4.0)
    z -= 0.6 * np.exp(-((u - 0.23 * W) ** 2 + (v - 0.26 * H) ** 2) / (2.0 * 40.0 ** 2))
    mid = (u >= 0.38 * W) & (u < 0.69 * W)
    z[mid] = 3.0 / (1.0 - 0.8 * dx[mid])
    floor = (u >= 0.69 * W) & (v > 0.61 * H)
    z[floor] = 1.2 / dy[floor]
    z[v >= 0.8 * H] = 30.0
    z *= 1.0 + 0.004 * rng.standard_normal((H, W))
    d = z.astype(np.float32)
    bad = rng.uniform(size=(H, W)) < 0.06
    d[bad] = rng.choice(np.array([0.0, np.nan, np.inf, -1.0], np.float32), size=int(bad.sum()))
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    kp = np.stack([rng.uniform(0.0, W - 1.0, M), rng.uniform(0.0, H - 1.0, M), rng.uniform(5.0, 150.0, M)], axis=1)
    return d, rgb, kp


def _stats(ms):
    ms = sorted(ms)
    return dict(median_us=1e3 * statistics.median(ms), p10_us=1e3 * ms[len(ms) // 10],
                p90_us=1e3 * ms[(9 * len(ms)) // 10], iters=len(ms))


def time_lift(ctx, d_depth, d_rgb, kp, mode, iters, warmup):
    from gcslam import _abi
    from gcslam.ops import VisualFeatureConfig
    from gcslam.ops.camera_features import _OUT, _cfg
    c_cfg = _cfg(VisualFeatureConfig(depth_sample_mode=mode))
    h_k = np.array([FX, FY, CX, CY])
    d_kp = _abi.DeviceArray.from_host(ctx, kp)
    out = _abi.alloc_many(ctx, [((M,) + shp, dt) for _, shp, dt in _OUT])

    def call():
        _abi.call("gc_camera_features_lift", ctx.handle, H, W, d_depth.ptr, d_rgb.ptr, M, d_kp.ptr, h_k.ctypes.data,
                  C.byref(c_cfg), *[o.ptr for o in out], ctx=ctx)

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
    names = [n for n, _, _ in _OUT]
    has_mu = out[names.index("has_mu_app")].download()
    Lc = out[names.index("depth_Lambda_c")].download()
    row = dict(what="gc_camera_features_lift", depth_sample_mode=mode, M=M, image=[W, H], **_stats(ms),
               valid_depth=int((Lc > 0.0).sum()), fitted=int(has_mu.sum()))
    print(json.dumps(row), flush=True)
    return row


def time_upload(ctx, name, arr, iters, warmup):
    from gcslam import _abi
    d = _abi.DeviceArray(ctx, arr.shape, arr.dtype)
    e0, e1 = _abi.Event(ctx), _abi.Event(ctx)
    for _ in range(warmup):
        d.upload(arr)
    ctx.sync()
    ms, wall = [], []
    for _ in range(iters):
        t0 = time.perf_counter()
        e0.record()
        d.upload(arr)
        e1.record()
        ctx.sync()
        wall.append(1e3 * (time.perf_counter() - t0))
        ms.append(e0.elapsed_ms(e1))
    s, w = _stats(ms), _stats(wall)
    row = dict(what="upload " + name, bytes=int(arr.nbytes), **s, host_median_us=w["median_us"],
               host_p10_us=w["p10_us"], host_p90_us=w["p90_us"], GBps=arr.nbytes / (s["median_us"] * 1e-6) / 1e9)
    print(json.dumps(row), flush=True)
    return d, row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=["median3", "hex"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from gcslam import _abi
    ctx = _abi.default_context()
    depth, rgb, kp = scene()
    d_depth, up_d = time_upload(ctx, "depth float32", depth, a.iters, a.warmup)
    d_rgb, up_c = time_upload(ctx, "rgb uint8", rgb, a.iters, a.warmup)
    rows = [up_d, up_c] + [time_lift(ctx, d_depth, d_rgb, kp, m, a.iters, a.warmup) for m in a.modes]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(image=[W, H], intrinsics=[FX, FY, CX, CY], rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
