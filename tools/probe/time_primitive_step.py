"""Time the scan step on the primitive map (gcslam.primitive_step.PrimitiveScanStep) at the reference's
shapes: K_HYP = 4 hypotheses, 8,192 points per scan, 7 active tiles (the radius-1 hex disk) of
m_tile = GC_M_TILE = 50,000 slots, M_TILE_VIEW = 1024, k_assoc = 8, the batch built from the scan
(budget -> deskew -> surfels, N = GC_N_FEAT + GC_N_SURFEL rows).

  run      host wall clock of one PrimitiveScanStep.run, the stream drained before and after;
  device   the pipeline's own launches of that run by its stage events (gc_pipeline_stage_ms): predict,
           k_pred_io, the span from k_pred_io's end to the evidence kernel's end (it contains the whole map
           branch front), combine_local, combine_final;
  stages   the same calls made one by one on a second pipeline and map that start equal, the stream
           drained after each: host wall clock per stage (its enqueue work plus its device time).

The two alternate in one loop. The scan's points are scaled into the map's extent so that the association
and the update have work to do (the counts are printed).

    python tools/probe/time_primitive_step.py [--iters 30] [--warmup 5] [--out FILE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gcslam import _abi, synth  # noqa: E402
from gcslam import primitive_map as PM  # noqa: E402
from gcslam.constants import GC_K_INSERT_TILE, GC_M_TILE  # noqa: E402
from gcslam.map_branch import MapBranch, MapBranchConfig  # noqa: E402
from gcslam.ops.deskew_constant_twist import deskew_constant_twist  # noqa: E402
from gcslam.ops.lidar_surfel_extraction import SurfelExtractionConfig, extract_lidar_surfels  # noqa: E402
from gcslam.ops.point_budget import point_budget_resample  # noqa: E402
from gcslam.pipeline import BatchedScanPipeline, PipelineConfig, iw_meas_prior, iw_process_prior  # noqa: E402
from gcslam.primitive_step import PrimitiveScanStep, lidar_cert_row, visual_cert  # noqa: E402
from time_map_branch import CENTER, build, fresh_map, summary  # noqa: E402

K_HYP, N_AZ, SCALE = 4, 512, 0.3  # 16 rings x 512 = 8,192 points; a 20 m room scaled to 6 m
STAGES = ("stage_front", "hyp0_download", "budget_deskew_surfels", "map_front", "evidence_back_finish", "map_update")


def make_pipeline(ctx, n):
    pipe = BatchedScanPipeline(K_HYP, n, PipelineConfig(n_points_cap=n), ctx=ctx)
    hy = synth.make_hypotheses(K_HYP)
    X = hy["X_anchor"].copy()
    X[:, 0:3] += CENTER
    pipe.set_beliefs(X, hy["z_lin"], hy["L"], hy["h"], hy["stamp"])
    pipe.set_weights(hy["weights"])
    pipe.set_io_evidence(*synth.make_io_evidence(K_HYP))
    pipe.set_iw(*iw_process_prior(), *iw_meas_prior())
    pipe.set_lidar_mode(True)
    return pipe


def staged_run(pipe, branch, scfg, slot, s, seq, t, acc):
    """PrimitiveScanStep.run's calls one by one, the stream drained after each."""
    ctx = pipe.ctx
    marks = [time.perf_counter()]

    def mark():
        ctx.sync()
        marks.append(time.perf_counter())
    pipe.stage_scan(slot, s)
    pipe.scan_front(slot, s, seq)
    mark()
    xi0, ess0, pp0 = pipe.front_hyp0()
    lin_d, _ = pipe.front_poses(device=True)
    mark()
    bud, _, _ = point_budget_resample(s["points"], s["timestamps"], s["weights"], n_points_cap=pipe.cfg.n_points_cap,
                                      chart_id=branch.chart_id, ctx=ctx, device_out=True)
    dsk, dc, _ = deskew_constant_twist(bud.points, bud.timestamps, bud.weights, float(s["scan_start"]),
                                       float(s["scan_end"]), xi0, ess0, branch.chart_id, "deskew_constant_twist",
                                       ctx=ctx, device_out=True)
    batch, sc, _ = extract_lidar_surfels(dsk.points, dsk.timestamps, dsk.weights, scfg, chart_id=branch.chart_id,
                                         ctx=ctx, device_out=True)
    mark()
    front = branch.front(batch, pp0[0:3].copy(), lin_d, seq, device_out=True)
    mark()
    row = lidar_cert_row([dc, sc, front.certs[1], visual_cert(front.vpe_cert, branch.config.eps_lift)], [front.certs[0]])
    pipe.set_lidar_evidence(front.device["L_lidar"], front.device["h_lidar"], row)
    pipe.scan_back()
    pipe.finish_scan()
    z_t = pipe.scan_map_pose()[0]
    mark()
    upd = branch.update(front, z_t, t)
    mark()
    if acc is not None:
        for name, a, b in zip(STAGES, marks, marks[1:]):
            acc[name].append(1e3 * (b - a))
    return upd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--m-tile", type=int, default=GC_M_TILE)
    ap.add_argument("--n-valid", type=int, default=4096, help="occupied slots per tile at the start")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _abi.default_context()
    rng = np.random.default_rng(0)
    keys, fields, _ = build(rng, a.m_tile, a.n_valid)
    scans = []
    for k in range(4):
        s = synth.make_scan(k, n_az=N_AZ)
        s["points"] = s["points"] * SCALE + CENTER * np.array([1.0, 1.0, 0.0])
        scans.append(s)
    n = scans[0]["points"].shape[0]
    cfg = MapBranchConfig(map_update=PM.MapUpdateConfig(k_insert_tile=GC_K_INSERT_TILE))
    scfg = SurfelExtractionConfig(voxel_size_m=0.25)
    maps = {w: fresh_map(ctx, keys, a.m_tile, a.n_valid, fields) for w in ("run", "stages")}
    pipes = {w: make_pipeline(ctx, n) for w in ("run", "stages")}
    pipes["run"].set_stage_timing(True)
    step = PrimitiveScanStep(pipes["run"], MapBranch(maps["run"], cfg), scfg)
    br2 = MapBranch(maps["stages"], cfg)
    run_ms, dev = [], {k: [] for k in ("predict_ms", "bins_ms", "evidence_ms", "combine_local_ms", "combine_final_ms")}
    acc = {k: [] for k in STAGES}
    counts = []
    for it in range(a.warmup + a.iters):
        s, slot, seq, t = scans[it % len(scans)], it % 3, 20 + it, 0.1 * it
        timed = it >= a.warmup
        ctx.sync()
        t0 = time.perf_counter()
        r = step.run(slot, s, seq, t)
        ctx.sync()
        if timed:
            run_ms.append(1e3 * (time.perf_counter() - t0))
            ms = pipes["run"].stage_ms()
            for k in dev:
                dev[k].append(ms[k])
        ctx.sync()
        u2 = staged_run(pipes["stages"], br2, scfg, slot, s, seq, t, acc if timed else None)
        counts.append((int(r.front.measurement_batch.n_lidar_valid), r.update[0].n_fused, r.update[0].n_inserted,
                       u2[0].n_fused == r.update[0].n_fused))
    res = dict(run=summary(run_ms), device={k: summary(v) for k, v in dev.items()},
               stages={k: summary(v) for k, v in acc.items()})
    fmt = lambda q: f"{q['median_ms']:.3f} ms [{q['p10_ms']:.3f}-{q['p90_ms']:.3f}]"  # noqa: E731
    lines = [f"shape: K_HYP = {K_HYP}, {n} points per scan, 7 active of {len(keys)} tiles, m_tile = {a.m_tile}, "
             f"M_TILE_VIEW = {cfg.M_TILE_VIEW}, k_assoc = {cfg.k_assoc}, k_insert_tile = {GC_K_INSERT_TILE}, "
             f"{a.n_valid} valid slots per tile at the start",
             f"load: valid surfels per scan {min(c[0] for c in counts)}-{max(c[0] for c in counts)}, fused rows "
             f"{min(c[1] for c in counts)}-{max(c[1] for c in counts)}, inserted {min(c[2] for c in counts)}-"
             f"{max(c[2] for c in counts)}; the two pipelines' fused counts equal on every scan: "
             f"{all(c[3] for c in counts)}",
             f"timing: host wall clock with the stream drained before and after each sample, device ms from the "
             f"pipeline's stage events; {a.warmup} warm-ups, median of {a.iters} [p10-p90]",
             f"PrimitiveScanStep.run, whole scan: {fmt(res['run'])}",
             f"  device, predict launch:            {fmt(res['device']['predict_ms'])}",
             f"  device, k_pred_io:                 {fmt(res['device']['bins_ms'])}",
             f"  device, k_pred_io end -> k_evidence_given end (holds the map branch front): "
             f"{fmt(res['device']['evidence_ms'])}",
             f"  device, combine_local:             {fmt(res['device']['combine_local_ms'])}",
             f"  device, combine_final:             {fmt(res['device']['combine_final_ms'])}",
             "the same calls one by one, the stream drained after each (host ms per stage):"]
    lines += [f"  {k:24s} {fmt(res['stages'][k])}" for k in STAGES]
    lines.append(f"  sum of the stages' medians: {sum(res['stages'][k]['median_ms'] for k in STAGES):.3f} ms")
    text = "\n".join(lines) + "\n" + json.dumps(res, indent=1) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
