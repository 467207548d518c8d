"""Time the maintenance of step 12b (backend/pipeline.py:1412-1447: cull, forget, merge-reduce of every
active tile) in two ways on one map, in one process:

  loop     the per-tile operators primitive_map_cull / primitive_map_forget / primitive_map_merge_reduce,
           one tile after the other, as primitive_map_update_from_association(maintenance=True) runs them:
           every cull and every merge-reduce waits for its counts;
  batched  primitive_map_maintain: one device pass over all active tiles (gc_primitive_map_maintain) and
           one download.

Each sample is the host wall clock of one whole maintenance, ending in a stream synchronise (what a
caller pays). The two alternate in one loop so drift hits both alike, after --warmup runs of each;
before every sample the map is restored from a pristine device copy, outside the timed window, so
every sample does the same work. Configurations:

  ref7, ref21   m_tile = GC_M_TILE (50,000) > GC_PRIMITIVE_MERGE_MAX_TILE_SIZE: the reference's
                configuration, where the merge is the budget-cap no-op (cull and forget only), at 7 and
                21 active tiles;
  merge7        m_tile = 2,048 with the merge on, 7 active tiles (2.1 M pair keys per tile).

    python tools/probe/time_map_maintain.py [--iters 20] [--warmup 3] [--configs ref7 ref21 merge7] [--json OUT]
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
from gcslam.constants import GC_M_TILE  # noqa: E402
from gcslam.primitive_map import (DevicePrimitiveMap, MapUpdateConfig, primitive_map_cull,  # noqa: E402
                                  primitive_map_forget, primitive_map_maintain, primitive_map_merge_reduce)

L = 3
CONFIGS = {"ref7": (GC_M_TILE, 7), "ref21": (GC_M_TILE, 21), "merge7": (2048, 7)}


def make_map(ctx, rng, m_tile, n_active):
    """n_active + 1 tiles (the last one inactive), 70 % of the slots valid, weights u^3."""
    n_tiles = n_active + 1
    M = n_tiles * m_tile
    B = rng.normal(size=(M, 3, 3))
    dm = DevicePrimitiveMap(n_tiles, m_tile, ctx=ctx)
    dm.upload(Lambdas=B @ np.swapaxes(B, 1, 2) + 0.5 * np.eye(3), thetas=rng.normal(size=(M, 3)) * 3.0,
              etas=rng.normal(size=(M, L, 3)), weights=rng.uniform(0, 1, M) ** 3, timestamps=rng.uniform(0, 5, M),
              created_timestamps=rng.uniform(0, 5, M), primitive_ids=np.arange(M, dtype=np.int64),
              valid_mask=(rng.uniform(0, 1, M) < 0.7).astype(np.uint8), cam_mass=rng.uniform(0, 1, M),
              lidar_mass=rng.uniform(0, 1, M), rgb_cam_accum=rng.uniform(0, 1, (M, 3)),
              rgb_cam_denom=rng.uniform(0, 1, M))
    return dm


def summary(s):
    s = sorted(s)
    return dict(median_ms=1e3 * statistics.median(s), p10_ms=1e3 * s[len(s) // 10], p90_ms=1e3 * s[(9 * len(s)) // 10],
                min_ms=1e3 * s[0], max_ms=1e3 * s[-1], spread_ms=1e3 * (s[(9 * len(s)) // 10] - s[len(s) // 10]),
                samples=len(s))


def time_config(name, iters, warmup):
    m_tile, n_active = CONFIGS[name]
    ctx = _abi.default_context()
    dm = make_map(ctx, np.random.default_rng(5), m_tile, n_active)
    cfg = MapUpdateConfig()
    dense = list(range(n_active))
    pristine = _abi.DeviceArray(ctx, dm.records.nbytes, np.uint8)
    nb = dm.slot_bytes

    def copy(dst, src):
        _abi.call("gc_copy_strided", ctx.handle, dst.ptr, nb, src.ptr, nb, nb, dm.M, ctx=ctx)

    copy(pristine, dm.records)
    counts = {d: 0 for d in dense}

    def restore():
        copy(dm.records, pristine)
        dm.tile_count, dm.total_count = dict(counts), 0
        ctx.sync()

    def loop():  # primitive_map_update_from_association(maintenance=True), its maintenance lines
        n_c = n_m = 0
        for d in dense:
            rc, _, _ = primitive_map_cull(dm, d, cfg.primitive_cull_weight_threshold)
            n_c += rc.n_culled
            primitive_map_forget(dm, d, cfg.primitive_forgetting_factor)
            rm, _, _ = primitive_map_merge_reduce(dm, d, cfg.primitive_merge_threshold, int(cfg.k_merge_pairs_tile),
                                                  int(cfg.max_tile_size), cfg.eps_psd, cfg.eps_lift,
                                                  anchor_id="primitive_map_merge_reduce")
            n_m += rm.n_merged
        ctx.sync()
        return n_c, n_m

    def batched():
        res, _, _ = primitive_map_maintain(dm, dense, cfg)
        ctx.sync()
        return res.n_culled_total, res.n_merged_total

    t = {"loop": [], "batched": []}
    outcome = {}
    for i in range(warmup + iters):
        for side, fn in (("loop", loop), ("batched", batched)):
            restore()
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            outcome.setdefault(side, out)
            assert outcome[side] == out
            if i >= warmup:
                t[side].append(dt)
    assert outcome["loop"] == outcome["batched"], outcome
    row = dict(config=name, m_tile=m_tile, n_active=n_active, merge_runs=not m_tile > cfg.max_tile_size,
               n_culled=int(outcome["loop"][0]), n_merged=int(outcome["loop"][1]), warmup=warmup,
               loop=summary(t["loop"]), batched=summary(t["batched"]))
    row["speedup_median"] = row["loop"]["median_ms"] / row["batched"]["median_ms"]
    row["batched_wins_by_more_than_loop_spread"] = bool(
        row["loop"]["median_ms"] - row["batched"]["median_ms"] > row["loop"]["spread_ms"])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = dict(clock="host perf_counter around one maintenance ending in a stream synchronise; loop and batched "
                     "alternate; the map is restored from a device copy before every sample",
               rows=[time_config(c, a.iters, a.warmup) for c in a.configs])
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
