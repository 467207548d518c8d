"""Time gc_extract_depth_surfels at DepthSurfelConfig's defaults (512 features, 1,024 surfels) on the
ray-cast floor-and-wall scene of tests/depth_surfel_cases.py with a seeded rgb: 640 x 480 with cell_px 16 and
1280 x 720 with cell_px 16 and 32. Each timed sample is one call between two events on the context's stream:
the call's two launches and its 4-byte row-count download, the images resident, outputs already allocated and
zeroed; warm-up calls first, then the median of --iters samples with p10 and p90.

Beside each time: the bytes the call must move at least (the depth image once, 3 B of rgb per used pixel, the
written rows) and the rate that implies. The call is launch- and latency-bound at these sizes.

    python tools/probe/time_depth_surfels.py [--iters 20] [--warmup 3] [--json OUT]
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
from gcslam.ops import DepthSurfelConfig  # noqa: E402
from gcslam.ops.camera_features import DEPTH_MODELS  # noqa: E402
import depth_surfel_cases as DC  # noqa: E402

SHAPES = ((480, 640, 16), (720, 1280, 16), (720, 1280, 32))


def time_extract(ctx, H, W, cell_px, iters, warmup):
    cfg = DepthSurfelConfig(cell_px=cell_px)
    depth, rgb, K = DC._scene(H, W, 0)
    dd = _abi.DeviceArray.from_host(ctx, depth, np.float32)
    dc = _abi.DeviceArray.from_host(ctx, rgb, np.uint8)
    n_total, L = cfg.n_feat + cfg.n_surfel, 3
    names = list(BATCH_ARRAYS)
    blk = _abi.alloc_many(ctx, [((n_total,) + (shp if k != "etas" else (L, 3)), BATCH_ARRAYS[k][2])
                                for k, (shp, _, _) in BATCH_ARRAYS.items()] + [((cfg.n_feat,), np.int32)])
    blk[0]._base.zero()
    ignored = dict(voxel_size_m=0.0, hex3d_num_cells_1=0.0, hex3d_num_cells_2=0.0, hex3d_num_cells_z=0.0,
                   hex3d_max_occupants=0.0, min_points_per_voxel=0.0, sensor_noise_var_per_axis=0.0)
    c_cfg = _abi.cfg("gc_surfel_cfg", cfg, n_lobes=L, **ignored)
    Kh, R, t = np.array(K, np.float64), np.ascontiguousarray(DC.R_BC), np.ascontiguousarray(DC.T_BC)
    nv = C.c_int32(0)

    def call():
        _abi.call("gc_extract_depth_surfels", ctx.handle, dd.ptr, dc.ptr, H, W, Kh.ctypes.data, R.ctypes.data,
                  t.ctypes.data, 0.0, 0, C.byref(c_cfg), int(cfg.cell_px), float(cfg.min_fill), float(cfg.min_depth_m),
                  float(cfg.max_depth_m), DEPTH_MODELS.index(cfg.depth_model), float(cfg.depth_sigma0),
                  float(cfg.depth_sigma_slope), float(cfg.plane_gate), float(cfg.min_cos_incidence),
                  float(cfg.weight_scale), *[b.ptr for b in blk[:len(names)]], blk[-1].ptr, C.byref(nv), ctx=ctx)

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
    used = int((np.isfinite(depth) & (depth > cfg.min_depth_m) & (depth < cfg.max_depth_m)).sum())
    moved = 4 * H * W + 3 * used + int(nv.value) * row_bytes
    n_cells = (-(-H // cell_px)) * (-(-W // cell_px))
    row = dict(H=H, W=W, cell_px=cell_px, n_cells=n_cells, n_rows=int(nv.value), median_us=1e3 * med,
               p10_us=1e3 * ms[len(ms) // 10], p90_us=1e3 * ms[(9 * len(ms)) // 10], iters=iters, min_bytes=moved,
               GBps=moved / (med * 1e-3) / 1e9)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = _abi.default_context()
    res = dict(config={k: v for k, v in DepthSurfelConfig().__dict__.items()},
               rows=[time_extract(ctx, H, W, c, a.iters, a.warmup) for H, W, c in SHAPES])
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
