"""Time the depth pose evidence (gcslam.ops.depth_pose_evidence_batched) at time_camera_render.py's shape:
640 x 480 pixels, tile_size 16, max_splats_per_tile 256, P = 1 and 4 poses, over maps of 10k and 100k
primitives, against a depth frame rendered at a slightly moved pose.

  prep      gc_camera_splat_prep;
  jvp       gc_camera_splat_jvp: the six tangents of every (pose, primitive);
  tiles     gc_render_depth_tiles: the forward lists and compositing, the floor of the evidence raster
            (the same exponential per (pixel, entry));
  evidence  gc_depth_pose_evidence: the evidence raster (k_ev_raster) and the per-pose sum (k_ev_final);
  whole     depth_pose_evidence_batched from a device batch, L, h and parts downloaded (host wall clock).

The first four are device times between events on the context's stream, the stream drained before each
sample; warm-ups first, then the median [p10-p90]. k_ev_raster against k_cam_raster alone is read from a
kernel trace of this script (rocprofv3 --kernel-trace --stats).

    python tools/probe/time_depth_evidence.py [--iters 10] [--warmup 2] [--poses 1 4] [--n 10000 100000] [--out FILE]
"""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "fl-slam_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gcslam import _abi  # noqa: E402
from gcslam import rendering as R  # noqa: E402
from gcslam.ops import DepthEvidenceConfig, depth_pose_evidence_batched  # noqa: E402
from time_camera_render import H, K, W, build, summary  # noqa: E402


def poses6(P):
    """P body poses [t, rotvec] on a short arc, all looking down +z."""
    out = np.zeros((P, 6))
    for p in range(P):
        out[p, 0] = 0.3 * p
        out[p, 4] = 0.04 * (p - 0.5 * (P - 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--poses", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--n", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _abi.default_context()
    vcfg, ecfg = R.CameraViewConfig(), DepthEvidenceConfig(robust_nu=4.0)
    c_cfg = R._camview_cfg(vcfg)
    ev = [_abi.Event(ctx) for _ in range(5)]
    names = ("prep", "jvp", "tiles", "evidence")
    lines, results = [], []
    for n in a.n:
        batch = R.DeviceRenderableBatch.from_host(ctx, build(np.random.default_rng(0), n))
        moved = np.array([[0.02, -0.015, 0.03, 0.004, -0.006, 0.003]])
        obs = R.render_map_camera(batch, K, R.camera_from_world(moved[0], ctx=ctx), H, W, vcfg).depth[0].astype(np.float32)
        d_obs = _abi.DeviceArray.from_host(ctx, obs, np.float32)
        for P in a.poses:
            X = poses6(P)
            T_cw = np.stack([R.camera_from_world(x, ctx=ctx) for x in X])
            t_wb, Ks = np.ascontiguousarray(X[:, :3]), [K] * P
            Kh = np.array([[K.fx, K.fy, K.cx, K.cy]] * P, np.float64)
            samples = {k: [] for k in names + ("whole",)}
            first = None
            for it in range(a.warmup + a.iters):
                dm, dz, dS, dL, dh, dp = _abi.alloc_many(ctx, [(P, n, 6, 2), (P, n, 6), (P, n, 6, 3), (P, 22, 22), (P, 22),
                                                               (P, _abi.GC_DEPTHEV_PARTS)])
                ctx.sync()
                ev[0].record()
                splats = R.camera_splat_prep(batch, Ks, T_cw, H, W, vcfg)
                st = R._CamSplatStruct(*[splats[k].ptr for k, _ in R._CamSplatStruct._fields_])
                ev[1].record()
                _abi.call("gc_camera_splat_jvp", ctx.handle, C.byref(batch.struct), n, P, T_cw.ctypes.data, t_wb.ctypes.data,
                          Kh.ctypes.data, H, W, C.byref(c_cfg), C.byref(st), dm.ptr, dz.ptr, dS.ptr, ctx=ctx)
                ev[2].record()
                dev = R.render_depth_tiles(splats, H, W, vcfg, ctx=ctx)
                ev[3].record()
                _abi.call("gc_depth_pose_evidence", ctx.handle, P, n, C.byref(st), dm.ptr, dz.ptr, dS.ptr, H, W,
                          int(vcfg.tile_size), int(vcfg.max_splats_per_tile), C.byref(c_cfg), dev["tile_counts"].ptr,
                          dev["tile_indices"].ptr, dev["alpha"].ptr, dev["depth"].ptr, d_obs.ptr, 0, ecfg.depth_sigma0,
                          ecfg.depth_sigma_slope, ecfg.min_depth_m, ecfg.max_depth_m, 1, ecfg.robust_nu, ecfg.eps_lift, 0,
                          dL.ptr, dh.ptr, dp.ptr, None, None, ctx=ctx)
                ev[4].record()
                ctx.sync()
                t0 = time.perf_counter()
                Lp, hp, parts, render = depth_pose_evidence_batched(batch, K, X, d_obs, view_cfg=vcfg, cfg=ecfg)
                dt = 1e3 * (time.perf_counter() - t0)
                if first is None:
                    first = parts.tobytes()
                assert parts.tobytes() == first and dp.download().tobytes() == first
                if it >= a.warmup:
                    for i, k in enumerate(names):
                        samples[k].append(ev[i].elapsed_ms(ev[i + 1]))
                    samples["whole"].append(dt)
            res = {k: summary(v) for k, v in samples.items()}
            surv, nc = dev["tile_survivors"].download(), dev["n_contrib"].download()
            res.update(n=n, poses=P, survivors_median=float(np.median(surv)), survivors_max=int(surv.max()),
                       tiles_at_cap=float((surv > vcfg.max_splats_per_tile).mean()), n_contrib_mean=float(nc.mean()),
                       n_used=[float(x) for x in parts[:, 43]], cost=[float(x) for x in parts[:, 42]])
            results.append(res)
            lines.append(f"{P} pose(s) of {W} x {H}, {n} primitives, tile_size {vcfg.tile_size}, cap "
                         f"{vcfg.max_splats_per_tile}: survivors per tile median {res['survivors_median']:.0f}, max "
                         f"{res['survivors_max']}; {100 * res['tiles_at_cap']:.1f} % of the tiles at the cap; "
                         f"{res['n_contrib_mean']:.1f} composited splats per pixel; {parts[0, 43]:.0f} pixels used at pose 0")
            for k, what in (("prep", "gc_camera_splat_prep (device, events)"), ("jvp", "gc_camera_splat_jvp (device, events)"),
                            ("tiles", "gc_render_depth_tiles (device, events)"),
                            ("evidence", "gc_depth_pose_evidence (device, events)"),
                            ("whole", "depth_pose_evidence_batched with the download (host clock)")):
                lines.append(f"  {what}: {res[k]['median_ms']:.3f} ms [{res[k]['p10_ms']:.3f}-{res[k]['p90_ms']:.3f}]")
    text = (f"timing: {a.warmup} warm-ups, median of {a.iters} [p10-p90]; the parts rows are identical bytes every run\n"
            + "\n".join(lines) + "\n" + json.dumps(results, indent=1) + "\n")
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
