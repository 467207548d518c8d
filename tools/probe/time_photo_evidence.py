"""Time the photometric and the joint RGB-D pose evidence at time_depth_evidence.py's shapes: 640 x 480 pixels,
tile_size 16, max_splats_per_tile 256, P = 1 and 4 poses, over maps of 10k and 100k primitives, against a
depth frame and an rgb image rendered at a slightly moved pose.

  shade   gc_camera_shade_jvp: the luminance and its six tangents of every (pose, primitive);
  depth   gc_depth_pose_evidence: k_ev_raster carrying the depth, and k_ev_final;
  photo   gc_photo_pose_evidence: k_ev_raster carrying the luminance, and k_ev_final;
  sum     depth + photo of the same iteration: the two single entries, what the joint entry replaces;
  rgbd    gc_rgbd_pose_evidence: one pass carrying both, and k_ev_final twice.

All are device times between events on the context's stream, in one session, the stream drained before each
sample; warm-ups first, then the median [p10-p90]. The prep, the tangents and the forward raster are made
once per shape by the first half of the wrappers' driver (camview_pose_evidence.prepare; time_depth_evidence.py
times them), and the entries are called as the driver calls them (evidence_call). The joint entry is the default of
rgbd_pose_evidence_batched only where its median is below the sum's by more than the two p10-p90 spreads
together: the last column says so per shape.

    python tools/probe/time_photo_evidence.py [--iters 20] [--warmup 3] [--poses 1 4] [--n 10000 100000] [--out FILE]
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "fl-slam_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gcslam import _abi  # noqa: E402
from gcslam import rendering as R  # noqa: E402
from gcslam.ops import DepthEvidenceConfig, PhotometricEvidenceConfig, luminance_image  # noqa: E402
from gcslam.ops import camview_pose_evidence as camview  # noqa: E402
from time_camera_render import H, K, W, build, summary  # noqa: E402
from time_depth_evidence import poses6  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--poses", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--n", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _abi.default_context()
    vcfg, ecfg, pcfg = R.CameraViewConfig(), DepthEvidenceConfig(robust_nu=4.0), PhotometricEvidenceConfig(robust_nu=4.0)
    ts, cap = int(vcfg.tile_size), int(vcfg.max_splats_per_tile)
    ev = [_abi.Event(ctx) for _ in range(5)]
    names = ("shade", "depth", "photo", "rgbd")
    lines, results = [], []
    for n in a.n:
        batch = R.DeviceRenderableBatch.from_host(ctx, build(np.random.default_rng(0), n))
        moved = np.array([0.02, -0.015, 0.03, 0.004, -0.006, 0.003])
        seen = R.render_map_camera(batch, K, R.camera_from_world(moved, ctx=ctx), H, W, vcfg)
        d_obs = _abi.DeviceArray.from_host(ctx, seen.depth[0].astype(np.float32), np.float32)
        rgb = np.clip(np.rint(seen.images[0] * 255.0), 0, 255).astype(np.uint8)
        l_obs = luminance_image(rgb, ctx=ctx, device_out=True)
        for P in a.poses:
            X = poses6(P)
            f = camview.prepare(batch, K, X, (d_obs, ecfg), (l_obs, pcfg), view_cfg=vcfg)   # the driver's first half
            dL, dh, pd, py, pj = _abi.alloc_many(ctx, [(P, 22, 22), (P, 22), (P, _abi.GC_DEPTHEV_PARTS),
                                                       (P, _abi.GC_DEPTHEV_PARTS), (P, 2, _abi.GC_DEPTHEV_PARTS)])
            dl, ddl = f.render["lum"], f.render["dlum"]
            samples = {k: [] for k in names + ("sum",)}
            first = None
            for it in range(a.warmup + a.iters):
                ctx.sync()
                ev[0].record()
                _abi.call("gc_camera_shade_jvp", ctx.handle, *f.views, f.weights.ctypes.data, dl.ptr, ddl.ptr, ctx=ctx)
                ev[1].record()
                camview.evidence_call(f, "depth", 0, dL, dh, pd)
                ev[2].record()
                camview.evidence_call(f, "photo", 0, dL, dh, py)
                ev[3].record()
                camview.evidence_call(f, "rgbd", 0, dL, dh, pj)
                ev[4].record()
                ctx.sync()
                rows = pj.download()
                assert rows[:, 0].tobytes() == pd.download().tobytes() and rows[:, 1].tobytes() == py.download().tobytes()
                if first is None:
                    first = rows.tobytes()
                assert rows.tobytes() == first
                if it >= a.warmup:
                    t = [ev[i].elapsed_ms(ev[i + 1]) for i in range(4)]
                    for k, x in zip(names, t):
                        samples[k].append(x)
                    samples["sum"].append(t[1] + t[2])
            res = {k: summary(v) for k, v in samples.items()}
            spread = lambda k: res[k]["p90_ms"] - res[k]["p10_ms"]
            joint_wins = res["rgbd"]["median_ms"] < res["sum"]["median_ms"] - (spread("rgbd") + spread("sum"))
            res.update(n=n, poses=P, n_used_depth=[float(x) for x in rows[:, 0, 43]],
                       n_used_photo=[float(x) for x in rows[:, 1, 43]], joint_below_sum_by_more_than_the_spreads=bool(joint_wins))
            results.append(res)
            lines.append(f"{P} pose(s) of {W} x {H}, {n} primitives, tile_size {ts}, cap {cap}: {rows[0, 0, 43]:.0f} depth and "
                         f"{rows[0, 1, 43]:.0f} luminance pixels used at pose 0")
            for k, what in (("shade", "gc_camera_shade_jvp"), ("depth", "gc_depth_pose_evidence"),
                            ("photo", "gc_photo_pose_evidence"), ("sum", "the two single entries"),
                            ("rgbd", "gc_rgbd_pose_evidence")):
                lines.append(f"  {what}: {res[k]['median_ms']:.3f} ms [{res[k]['p10_ms']:.3f}-{res[k]['p90_ms']:.3f}]")
            lines.append(f"  joint / sum = {res['rgbd']['median_ms'] / res['sum']['median_ms']:.3f}; joint below the sum by more "
                         f"than the two spreads: {'yes' if joint_wins else 'no'}")
    text = (f"timing: {a.warmup} warm-ups, median of {a.iters} [p10-p90], device ms between events; the joint rows are the "
            "single entries' bytes every run\n" + "\n".join(lines) + "\n" + json.dumps(results, indent=1) + "\n")
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
