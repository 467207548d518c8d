"""Time gc_camera_measurement_batch at the reference's budget (M = 512 features, n_feat = 512,
n_surfel = 1,024, the default LidarCameraDepthFusionConfig: radius 3 px, 64 fitted points) for
N = 8,192 points (GC_N_POINTS_CAP) and N = 65,536 on a 640 x 480 image (fx = fy = 500). The scene is
that of tests/camsplat_cases.py at this image size: pixels uniform over the image, a 4 m wall, a
slanted wall, a floor and a far wall, 1/16 of the points behind the camera. Each timed sample is one
call between two events on the context's stream: its memset, three launches and the 4-byte
candidate-cap download, inputs resident and outputs allocated; warm-up calls first, then the median
of --iters samples.

Beside each time, the bytes the call must move at least: k_cs_project reads 24 B and writes 40 B per
point; k_cs_query reads 16 B per (query, point) pair (from L2: the projected pixels are 1 MB at
N = 65,536) and 24 B per candidate; k_cs_finish reads about 250 B per feature and writes 217 B per
batch row.

With --reference PATH the reference's own NumPy lidar_depth_evidence (the O(M N) part of
splat_prep_fused) is timed on the same inputs on this machine's CPU instead (no GPU is touched): the
median of --iters calls.

    python tools/probe/time_camera_splats.py [--iters 200] [--sizes 8192 65536] [--json OUT]
    python tools/probe/time_camera_splats.py --reference /path/to/reference --iters 5 [--json OUT]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import camsplat_cases as CC  # noqa: E402

W, H, FX, FY, CX, CY = 640.0, 480.0, 500.0, 500.0, 320.0, 240.0
M = 512


def scene(n, seed=0):
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0.0, W, n), rng.uniform(0.0, H, n)
    dx, dy = (u - CX) / FX, (v - CY) / FY
    z = np.full(n, 4.0)
    mid = (u >= 0.38 * W) & (u < 0.69 * W)
    z[mid] = 3.0 / (1.0 - 0.8 * dx[mid])
    floor = (u >= 0.69 * W) & (v > 0.61 * H)
    z[floor] = 1.2 / dy[floor]
    z[v >= 0.8 * H] = 30.0
    z = z + rng.standard_normal(n) * (0.01 * z / 4.0)
    p = np.stack([dx * z, dy * z, z], axis=1)
    p[: n // 16] *= -1.0
    uv = np.stack([rng.uniform(0.0, W, M), rng.uniform(0.0, H, M)], axis=1)
    return p @ CC.R_BASE_CAMERA.T + CC.T_BASE_CAMERA, uv


def time_device(n, iters, warmup):
    from gcslam import _abi
    from gcslam.constants import GC_EPS_LIFT, GC_N_FEAT, GC_N_SURFEL, GC_VMF_N_LOBES
    from gcslam.measurement_batch import BATCH_ARRAYS
    from gcslam.ops import LidarCameraDepthFusionConfig
    from gcslam.ops.camera_splats import _cfg
    ctx = _abi.default_context()
    base, uv = scene(n)
    f = CC.features(uv)
    dp = _abi.DeviceArray.from_host(ctx, base)
    order = [uv, f["depth_Lambda_c"], f["depth_theta_c"], f["weight"], f["kappa_app"], f["mu_app"],
             f["has_mu_app"].astype(np.uint8), f["color"], f["has_color"].astype(np.uint8), f["xyz"], f["cov_xyz"]]
    dev = _abi.upload_many(ctx, order, [np.uint8 if a.dtype == np.uint8 else np.float64 for a in order])
    n_total, L = GC_N_FEAT + GC_N_SURFEL, GC_VMF_N_LOBES
    blk = _abi.alloc_many(ctx, [((n_total,) + (shp if k != "etas" else (L, 3)), BATCH_ARRAYS[k][2])
                                for k, (shp, _, _) in BATCH_ARRAYS.items()] +
                          [((M, 3), np.float64), ((M, 3, 3), np.float64), ((M,), np.uint8), ((M, _abi.GC_CAM_EV), np.float64),
                           ((M,), np.int32)])
    c_cfg = _cfg(LidarCameraDepthFusionConfig())
    h_k = np.array([FX, FY, CX, CY])
    R, t = np.ascontiguousarray(CC.R_BASE_CAMERA), np.ascontiguousarray(CC.T_BASE_CAMERA)

    def call():
        _abi.call("gc_camera_measurement_batch", ctx.handle, n, dp.ptr, R.ctypes.data, t.ctypes.data, M,
                  *[d.ptr for d in dev], h_k.ctypes.data, C.byref(c_cfg), 1.0, 0.5, GC_N_FEAT, GC_N_SURFEL, L,
                  GC_EPS_LIFT, *[b.ptr for b in blk], ctx=ctx)

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
    cnt = blk[-1].download()
    flag = blk[-3].download()
    moved = dict(project=n * 64, query=M * n * 16 + int(cnt.sum()) * 24, finish=M * 250 + n_total * 217)
    row = dict(N=n, M=M, median_us=1e3 * med, p10_us=1e3 * ms[len(ms) // 10], p90_us=1e3 * ms[(9 * len(ms)) // 10],
               iters=iters, in_radius_median=float(np.median(cnt)), in_radius_max=int(cnt.max()),
               supported_queries=int((cnt >= 3).sum()), fused_rows=int(flag.sum()), min_bytes=moved,
               query_GBps=moved["query"] / (med * 1e-3) / 1e9)
    print(json.dumps(row), flush=True)
    return row


def time_reference(ref_root, n, iters):
    sys.path.insert(0, os.path.join(ref_root, "fl_ws", "src", "fl_slam_poc"))
    from fl_slam_poc.frontend.sensors import lidar_camera_depth_fusion as F
    import camsplat_restatement as RS
    base, uv = scene(n)
    pc = RS.to_camera_frame(base, CC.R_BASE_CAMERA, CC.T_BASE_CAMERA)
    cfg = F.LidarCameraDepthFusionConfig()
    s = []
    for _ in range(iters):
        t0 = time.perf_counter()
        F.lidar_depth_evidence(pc, uv, FX, FY, CX, CY, cfg)
        s.append(time.perf_counter() - t0)
    row = dict(N=n, M=M, reference_numpy_lidar_depth_evidence_s=statistics.median(s), min_s=min(s), max_s=max(s),
               iters=iters, cpus=os.cpu_count())
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 65536])
    ap.add_argument("--reference", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.reference:
        res = dict(rows=[time_reference(a.reference, n, a.iters) for n in a.sizes])
    else:
        res = dict(image=[W, H], intrinsics=[FX, FY, CX, CY],
                   rows=[time_device(n, a.iters, a.warmup) for n in a.sizes])
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
