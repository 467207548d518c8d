"""Time one post-pose map update (backend/pipeline.py:1232-1492, step 12b) at the reference's per-scan
shape: N = 1536 measurement primitives (512 features + 1024 surfels), K = 8 candidates, 7 active
tiles (the radius-1 hex disk) of m_tile = GC_M_TILE slots, k_insert_tile = GC_K_INSERT_TILE, in two
ways on two maps that start equal:

  fused    primitive_map_update_from_association: one device pass (gc_primitive_map_update), one download;
  dropins  the same step composed from the per-tile drop-ins (tests/mapupdate_dropins.py): 6 blocks x 7
           tiles of primitive_map_fuse on repeated rows, the plan in NumPy, 7 primitive_map_insert_masked.

Each sample is the host wall clock of one whole update, host work and waits included (what a caller
pays); the two alternate in one loop so drift hits both alike, after --warmup updates of each. Both
maps keep evolving (every update inserts), which is the steady state of a running node. With
--maintenance the per-tile cull / forget / merge-reduce (the same entries on both sides) is included;
at m_tile = GC_M_TILE > GC_PRIMITIVE_MERGE_MAX_TILE_SIZE the merge is the reference's budget-cap no-op.

The association is synthetic (its numbers do not matter to the time): every row's candidates are
valid slots of the tile its world mean falls in or of a neighbour, about a third name tiles outside
the active set, and a third of the valid rows carry novelty > 0.

    python tools/probe/time_map_update.py [--iters 30] [--warmup 5] [--maintenance] [--json OUT]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gcslam import _abi, tiling  # noqa: E402
from gcslam.constants import GC_H_TILE, GC_K_INSERT_TILE, GC_M_TILE, GC_N_FEAT, GC_N_SURFEL  # noqa: E402
from gcslam.primitive_map import (DevicePrimitiveMap, MapUpdateConfig,  # noqa: E402
                                  primitive_map_update_from_association)

L = 3


class _Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def build_inputs(rng, N, K, m_tile, n_valid):
    """(tile keys of the map, active keys, initial map fields, meas, assoc, pose)."""
    h = GC_H_TILE
    active = tiling.ma_hex_stencil_tile_ids(np.array([0.5, 0.5, 0.5]), h, 1, 0)
    ring2 = tiling.ma_hex_stencil_tile_ids(np.array([0.5, 0.5, 0.5]), h, 2, 0)
    keys = active + [k for k in ring2 if k not in active]  # 19 tiles in the map, 7 active
    M = len(keys) * m_tile
    B = rng.normal(size=(M, 3, 3)) * 0.3
    Lam = B @ np.swapaxes(B, 1, 2) + 2.0 * np.eye(3)
    valid = np.zeros(M, np.uint8)
    for d in range(len(keys)):
        valid[d * m_tile:d * m_tile + n_valid] = 1
    fields = dict(Lambdas=Lam, thetas=np.einsum("nij,nj->ni", Lam, rng.uniform(-4.0, 6.0, (M, 3))),
                  etas=rng.normal(size=(M, L, 3)) * 2.0, weights=rng.uniform(0.1, 1.0, M) * valid,
                  valid_mask=valid, primitive_ids=np.arange(M, dtype=np.int64),
                  last_supported_scan_seq=rng.integers(0, 12, M))
    pos = np.column_stack([rng.uniform(-3.0, 5.0, N), rng.uniform(-3.0, 5.0, N), rng.uniform(0.0, 2.0, N)])
    vm = rng.uniform(0, 1, N) < 0.85
    meas = dict(Lambdas=np.tile(4.0 * np.eye(3), (N, 1, 1)), thetas=4.0 * pos, etas=rng.normal(size=(N, L, 3)) * 2.0,
                weights=rng.uniform(0.1, 1.0, N), valid_mask=vm, colors=rng.uniform(0, 1, (N, 3)),
                sources=(np.arange(N) >= GC_N_FEAT).astype(np.int32))
    pose = np.array([0.05, -0.03, 0.0, 0.0, 0.0, 0.04])
    own = tiling.tile_ids_from_xyz_batch(pos, h)
    ctile = np.where(rng.uniform(0, 1, (N, K)) < 0.6, own[:, None], rng.choice(np.asarray(keys), (N, K)))
    resp = rng.uniform(0, 1, (N, K)) / (N * K) * vm[:, None]
    a = 1.0 / max(int(vm.sum()), 1)
    rm = np.where(rng.uniform(0, 1, N) < 1.0 / 3.0, rng.uniform(0, 0.9, N) * a, 50.0 * a)
    assoc = dict(responsibilities=resp, candidate_pool_indices=np.zeros((N, K), np.int32), candidate_tile_ids=ctile,
                 candidate_slots=rng.integers(0, n_valid, (N, K)), row_masses=rm, cost_matrix=np.zeros((N, K)))
    return keys, active, fields, meas, assoc, pose


def fresh_map(ctx, keys, m_tile, n_valid, fields):
    dm = DevicePrimitiveMap(len(keys), m_tile, ctx=ctx)
    dm.set_tile_keys(keys)
    dm.upload(**fields)
    dm.tile_count = {d: n_valid for d in range(len(keys))}
    dm.total_count = n_valid * len(keys)
    dm.next_global_id = len(keys) * m_tile
    return dm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--m-tile", type=int, default=GC_M_TILE)
    ap.add_argument("--n-valid", type=int, default=4096, help="occupied slots per tile at the start")
    ap.add_argument("--maintenance", action="store_true")
    ap.add_argument("--only", choices=("fused", "dropins"), default=None, help="one side alone (kernel traces)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from mapupdate_dropins import dropin_map_update
    from gcslam.association import PrimitiveAssociationResult
    ctx = _abi.default_context()
    rng = np.random.default_rng(0)
    N, K = GC_N_FEAT + GC_N_SURFEL, 8
    keys, active, fields, meas, assoc, pose = build_inputs(rng, N, K, a.m_tile, a.n_valid)
    cfg = MapUpdateConfig(k_insert_tile=GC_K_INSERT_TILE)
    cfg_d = dict(k_insert_tile=GC_K_INSERT_TILE, block_size=cfg.block_size, h_tile=cfg.h_tile)
    sides = [s for s in ("fused", "dropins") if a.only in (None, s)]
    maps = {s: fresh_map(ctx, keys, a.m_tile, a.n_valid, fields) for s in sides}
    res_a, batch = PrimitiveAssociationResult(**assoc), _Obj(**meas)
    samples = {s: [] for s in sides}
    last = {}
    for it in range(a.warmup + a.iters):
        seq = 20 + it
        for s in sides:
            ctx.sync()
            t0 = time.perf_counter()
            if s == "fused":
                r, _, _ = primitive_map_update_from_association(maps[s], res_a, batch, active, pose, 0.1 * it, seq, cfg,
                                                                maintenance=a.maintenance)
                last[s] = dict(n_fused=r.n_fused, n_inserted=r.n_inserted, n_culled=r.n_culled)
            else:
                r = dropin_map_update(maps[s], assoc, meas, active, pose, 0.1 * it, seq, cfg_d, a.maintenance)
                last[s] = {k: r[k] for k in ("n_fused", "n_inserted", "n_culled")}
            ctx.sync()
            if it >= a.warmup:
                samples[s].append(1e3 * (time.perf_counter() - t0))
    out = dict(shape=dict(N=N, K=K, n_active=len(active), n_tiles=len(keys), m_tile=a.m_tile,
                          k_insert_tile=GC_K_INSERT_TILE, n_valid_start=a.n_valid, block_size=cfg.block_size),
               maintenance=bool(a.maintenance), timing="host wall clock per update, stream drained before and after",
               last_counters=last)
    for s, v in samples.items():
        v.sort()
        out[s] = dict(median_ms=statistics.median(v), p10_ms=v[len(v) // 10], p90_ms=v[(9 * len(v)) // 10],
                      iters=a.iters)
        print(json.dumps({s: out[s]}), flush=True)
    if len(sides) == 2:
        out["sides_agree"] = last["fused"] == last["dropins"]
        print(json.dumps({"sides_agree": out["sides_agree"], "last_counters": last}), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
