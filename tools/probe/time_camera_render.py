"""Time the camera view (gcslam.rendering.render_map_camera) at the viewer's shape: 640 x 480 pixels,
tile_size 16, max_splats_per_tile 256, one view and eight views, over maps of 10k and 100k primitives
spread in front of the cameras so that typical tiles hold tens to a few hundred survivors.

  prep     gc_camera_splat_prep: the mass maximum and the 2D splats of every view;
  tiles    gc_render_depth_tiles: the depth-ordered tile lists (k_cam_bin_select) and the compositing
           (k_cam_raster);
  whole    render_map_camera from a device batch, everything downloaded (host wall clock).

prep and tiles are device times between two events on the context's stream, the stream drained before
each sample; warm-ups first, then the median [p10-p90]. The lists and the compositing are one entry:
their split is read from a kernel trace of this script (rocprofv3 --kernel-trace --stats),
k_cam_bin_select against k_cam_raster. The share of tiles at the cap (tile_survivors > cap) is reported.

    python tools/probe/time_camera_render.py [--iters 10] [--warmup 2] [--views 1 8] [--n 10000 100000] [--out FILE]
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "fl-slam_amd"))
sys.path.insert(0, ROOT)

from gcslam import _abi  # noqa: E402
from gcslam import rendering as R  # noqa: E402
from gcslam.ops.camera_splats import PinholeIntrinsics  # noqa: E402

L = 3
H, W = 480, 640
K = PinholeIntrinsics(500.0, 500.0, 320.0, 240.0)


def build(rng, n):
    """n primitives at 2 .. 30 m over the frame and a little beyond; sigma shrinks with the map's density
    (as a denser map's surfels do), 5 .. 25 cm at 10k."""
    s = (10000.0 / n) ** 0.5
    Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    ev = np.exp(rng.uniform(np.log(0.05 * s), np.log(0.25 * s), (n, 3))) ** 2
    Sigma = np.einsum("nij,nj,nkj->nik", Q, ev, Q)
    z = rng.uniform(2.0, 30.0, n)
    mu = np.column_stack([rng.uniform(-0.75, 0.75, n) * z, rng.uniform(-0.6, 0.6, n) * z, z])
    return R.RenderablePrimitiveBatch(mu_world=mu, Sigma_world=0.5 * (Sigma + np.swapaxes(Sigma, 1, 2)), Lambda_world=None,
                                      eta=rng.normal(size=(n, L, 3)) * 2.0, mass=rng.uniform(0.1, 1.0, n),
                                      color=rng.uniform(0.0, 1.0, (n, 3)), primitive_ids=np.arange(n, dtype=np.int64))


def poses(nv):
    """nv cameras on a short arc around the origin, all looking down +z."""
    out = []
    for v in range(nv):
        a = 0.04 * (v - 0.5 * (nv - 1))
        T_wb = np.eye(4)
        T_wb[:3, :3] = [[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]
        T_wb[:3, 3] = [0.3 * v, 0.0, 0.0]
        out.append(R.camera_from_world(T_wb))
    return np.stack(out)


def summary(v):
    v = sorted(v)
    return dict(median_ms=statistics.median(v), p10_ms=v[len(v) // 10], p90_ms=v[(9 * len(v)) // 10], n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--views", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--n", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _abi.default_context()
    cfg = R.CameraViewConfig()
    e0, e1, e2 = _abi.Event(ctx), _abi.Event(ctx), _abi.Event(ctx)
    lines, results = [], []
    for n in a.n:
        batch = R.DeviceRenderableBatch.from_host(ctx, build(np.random.default_rng(0), n))
        for nv in a.views:
            T_cw, Ks = poses(nv), [K] * nv
            samples = dict(prep=[], tiles=[], whole=[])
            first = None
            for it in range(a.warmup + a.iters):
                ctx.sync()
                e0.record()
                splats = R.camera_splat_prep(batch, Ks, T_cw, H, W, cfg)
                e1.record()
                dev = R.render_depth_tiles(splats, H, W, cfg, ctx=ctx)
                e2.record()
                ctx.sync()
                t0 = time.perf_counter()
                out = R.render_map_camera(batch, Ks, T_cw, H, W, cfg)
                dt = 1e3 * (time.perf_counter() - t0)
                if first is None:
                    first = out.images.tobytes()
                assert out.images.tobytes() == first and dev["images"].download().tobytes() == first
                if it >= a.warmup:
                    samples["prep"].append(e0.elapsed_ms(e1))
                    samples["tiles"].append(e1.elapsed_ms(e2))
                    samples["whole"].append(dt)
            res = {k: summary(v) for k, v in samples.items()}
            res.update(n=n, views=nv, survivors_mean=float(out.tile_survivors.mean()),
                       survivors_median=float(np.median(out.tile_survivors)), survivors_max=int(out.tile_survivors.max()),
                       tiles_at_cap=float((out.tile_survivors > cfg.max_splats_per_tile).mean()),
                       n_contrib_mean=float(out.n_contrib.mean()), coverage_mean=float(out.alpha.mean()))
            results.append(res)
            lines.append(f"{nv} view(s) of {W} x {H}, {n} primitives, tile_size {cfg.tile_size}, cap "
                         f"{cfg.max_splats_per_tile}: survivors per tile median {res['survivors_median']:.0f}, mean "
                         f"{res['survivors_mean']:.1f}, max {res['survivors_max']}; {100 * res['tiles_at_cap']:.1f} % of the "
                         f"tiles at the cap; {res['n_contrib_mean']:.1f} composited splats per pixel")
            for k, what in (("prep", "gc_camera_splat_prep (device, events)"),
                            ("tiles", "gc_render_depth_tiles (device, events)"),
                            ("whole", "render_map_camera with the download (host clock)")):
                lines.append(f"  {what}: {res[k]['median_ms']:.3f} ms [{res[k]['p10_ms']:.3f}-{res[k]['p90_ms']:.3f}]")
    text = (f"timing: {a.warmup} warm-ups, median of {a.iters} [p10-p90]; the images are identical bytes every run\n"
            + "\n".join(lines) + "\n" + json.dumps(results, indent=1) + "\n")
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
