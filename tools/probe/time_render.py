"""Time render_map_bev (gcslam.rendering) at a map-sized shape: 15 views (BEV15) of 512 x 512 pixels
over 16,384 primitives, tile_size 32, max_splats_per_tile 64 (SplatRenderingConfig's defaults).

  prep     gc_bev_splat_prep: the 2D splats of every view;
  tiles    gc_render_ewa_tiles: the tile binning (key, segmented sort and take kernels) and the raster;
  whole    render_map_bev from a device batch, the images downloaded (host wall clock).

prep and tiles are device times between two events on the context's stream, the stream drained
before each sample; warm-ups first, then the median [p10-p90]. The binning and the raster are one
entry: their split is read from a kernel trace of this script (rocprofv3 --kernel-trace --stats),
k_raster against k_bin_keys + k_bin_take + the k_sort_* kernels.

    python tools/probe/time_render.py [--iters 20] [--warmup 3] [--views 15] [--size 512] [--n 16384] [--out FILE]
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

L = 3


def build(rng, n, extent_m):
    """n primitives spread over the viewport: sigma 5 .. 25 cm, as a settled map's surfels."""
    Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    ev = np.exp(rng.uniform(np.log(0.0025), np.log(0.0625), (n, 3)))
    Sigma = np.einsum("nij,nj,nkj->nik", Q, ev, Q)
    mu = np.column_stack([rng.uniform(0.0, extent_m, n), rng.uniform(0.0, extent_m, n), rng.uniform(-0.5, 2.0, n)])
    return R.RenderablePrimitiveBatch(mu_world=mu, Sigma_world=0.5 * (Sigma + np.swapaxes(Sigma, 1, 2)), Lambda_world=None,
                                      eta=rng.normal(size=(n, L, 3)) * 2.0, mass=rng.uniform(0.1, 1.0, n),
                                      color=rng.uniform(0.0, 1.0, (n, 3)), primitive_ids=np.arange(n, dtype=np.int64))


def summary(v):
    v = sorted(v)
    return dict(median_ms=statistics.median(v), p10_ms=v[len(v) // 10], p90_ms=v[(9 * len(v)) // 10], n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--views", type=int, default=15)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--px-per-m", type=float, default=16.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _abi.default_context()
    cfg, bcfg = R.SplatRenderingConfig(), R.BEVPushforwardConfig(n_views=a.views)
    vp = R.Viewport((0.0, 0.0), a.px_per_m, a.size, a.size)
    batch = R.DeviceRenderableBatch.from_host(ctx, build(np.random.default_rng(0), a.n, a.size / a.px_per_m))
    P, vd = R.bev_views(bcfg, "bev15")
    e0, e1, e2 = _abi.Event(ctx), _abi.Event(ctx), _abi.Event(ctx)
    samples = dict(prep=[], tiles=[], whole=[])
    first = None
    for it in range(a.warmup + a.iters):
        ctx.sync()
        e0.record()
        splats = R.bev_splat_prep(batch, vp, P, vd, cfg, fbm_modulate_scale=0.3)
        e1.record()
        dev = R.render_ewa_tiles(splats, a.size, a.size, cfg.tile_size, cfg.max_splats_per_tile, cfg.ewa_log_clip,
                                 cfg.eps, ctx=ctx)
        e2.record()
        ctx.sync()
        t0 = time.perf_counter()
        out = R.render_map_bev(batch, vp, cfg, bcfg, "bev15", fbm_modulate_scale=0.3)
        dt = 1e3 * (time.perf_counter() - t0)
        if first is None:
            first = out.images.tobytes()
        assert out.images.tobytes() == first and dev["images"].download().tobytes() == first
        if it >= a.warmup:
            samples["prep"].append(e0.elapsed_ms(e1))
            samples["tiles"].append(e1.elapsed_ms(e2))
            samples["whole"].append(dt)
    res = {k: summary(v) for k, v in samples.items()}
    T = (a.size // cfg.tile_size) ** 2
    res["tile_count_mean"] = float(out.tile_counts.mean())
    res["tiles_at_cap"] = float((out.tile_counts == cfg.max_splats_per_tile).mean())
    lines = [f"shape: {a.views} views of {a.size} x {a.size}, {a.n} primitives, tile_size {cfg.tile_size} "
             f"({T} tiles per view), cap {cfg.max_splats_per_tile}; mean list length {res['tile_count_mean']:.1f}, "
             f"{100 * res['tiles_at_cap']:.0f} % of the tiles at the cap",
             f"timing: {a.warmup} warm-ups, median of {a.iters} [p10-p90]; the images are identical bytes every run"]
    for k, what in (("prep", "gc_bev_splat_prep (device, events)"), ("tiles", "gc_render_ewa_tiles (device, events)"),
                    ("whole", "render_map_bev with the download (host clock)")):
        lines.append(f"{what}: {res[k]['median_ms']:.3f} ms [{res[k]['p10_ms']:.3f}-{res[k]['p90_ms']:.3f}]")
    text = "\n".join(lines) + "\n" + json.dumps(res, indent=1) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
