"""Time the map branch of one scan (gcslam.map_branch.MapBranch) at the reference's shapes: N = 1536
measurement primitives, 7 active tiles (the radius-1 hex disk) of m_tile = GC_M_TILE = 50,000 slots,
M_TILE_VIEW = 1024, k_assoc = 8, k_insert_tile = GC_K_INSERT_TILE, H = 2 hypothesis poses.

  branch   MapBranch.front + MapBranch.update: ensure_tiles (all hits here), the batched recency
           inflate, view, association, candidate statistics, batched pose evidence, step 12b;
  hand     the same operators composed by hand as before MapBranch existed: the per-tile
           primitive_map_recency_inflate (one call, wait and download per tile) and no candidate
           statistics.

The two run on two maps that start equal and alternate in one loop; each sample is the host wall
clock of one whole scan with the stream drained before and after. Then, on a map of 7 slabs:

  swap3    one ensure_tiles call that replaces 3 of the 7 resident tiles (3 exports to the host store,
           3 imports from it, one wait); the wanted set alternates between two stencils 3 tiles apart;
  allhit   one ensure_tiles call whose 7 keys are all resident (host clock of the call alone, and the
           same with a synchronise after it).

    python tools/probe/time_map_branch.py [--iters 20] [--warmup 3] [--out FILE]
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

from gcslam import _abi, tiling  # noqa: E402
from gcslam import primitive_map as PM  # noqa: E402
from gcslam.association import associate_primitives_ot, extract_atlas_map_view  # noqa: E402
from gcslam.constants import GC_H_TILE, GC_K_INSERT_TILE, GC_M_TILE, GC_N_FEAT, GC_N_SURFEL  # noqa: E402
from gcslam.map_branch import MapBranch, MapBranchConfig  # noqa: E402
from gcslam.ops import visual_pose_evidence_batched  # noqa: E402

L = 3
CENTER = np.array([0.5, 0.5, 0.5])


class _Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _cell_positions(rng, key_cells, n):
    """n positions inside each MA-hex cell (c1, c2, cz): s1 = x, s2 = x / 2 + y sqrt(3) / 2."""
    out = []
    h = GC_H_TILE
    for c1, c2, cz in key_cells:
        s1 = rng.uniform(c1 * h, (c1 + 1) * h, n)
        s2 = rng.uniform(c2 * h, (c2 + 1) * h, n)
        out.append(np.column_stack([s1, (s2 - 0.5 * s1) / (np.sqrt(3.0) * 0.5), rng.uniform(cz * h, (cz + 1) * h, n)]))
    return np.concatenate(out)


def build(rng, m_tile, n_valid):
    c0 = tiling.tile_cells_from_xyz_batch(CENTER, GC_H_TILE)[0]
    cells = [(int(c0[0]) + q, int(c0[1]) + r, int(c0[2])) for q, r in tiling.hex_disk_axial(2)]
    keys = [tiling.tile_id_from_cell_3d(*c) for c in cells]  # 19 tiles, the 7 active among them
    M = len(keys) * m_tile
    B = rng.normal(size=(M, 3, 3)) * 0.3
    Lam = B @ np.swapaxes(B, 1, 2) + 2.0 * np.eye(3)
    valid = np.zeros(M, np.uint8)
    for d in range(len(keys)):
        valid[d * m_tile:d * m_tile + n_valid] = 1
    pos = _cell_positions(rng, cells, m_tile)
    fields = dict(Lambdas=Lam, thetas=np.einsum("nij,nj->ni", Lam, pos), etas=rng.normal(size=(M, L, 3)) * 2.0,
                  weights=rng.uniform(0.1, 1.0, M) * valid, valid_mask=valid,
                  primitive_ids=np.arange(M, dtype=np.int64), last_supported_scan_seq=rng.integers(0, 12, M))
    N = GC_N_FEAT + GC_N_SURFEL
    mp = np.column_stack([rng.uniform(-2.0, 3.0, N), rng.uniform(-2.0, 3.0, N), rng.uniform(0.0, 2.0, N)])
    meas = dict(Lambdas=np.tile(4.0 * np.eye(3), (N, 1, 1)), thetas=4.0 * mp, etas=rng.normal(size=(N, L, 3)) * 2.0,
                weights=rng.uniform(0.1, 1.0, N), valid_mask=rng.uniform(0, 1, N) < 0.85,
                colors=rng.uniform(0, 1, (N, 3)), sources=(np.arange(N) >= GC_N_FEAT).astype(np.int32))
    return keys, fields, meas


def fresh_map(ctx, keys, m_tile, n_valid, fields, n_tiles=None):
    n = n_tiles or len(keys)
    dm = PM.DevicePrimitiveMap(n, m_tile, ctx=ctx)
    dm.set_tile_keys(keys[:n])
    dm.upload(**{k: v[:n * m_tile] for k, v in fields.items()})
    dm.tile_count = {d: n_valid for d in range(n)}
    dm.total_count = n_valid * n
    dm.next_global_id = len(keys) * m_tile
    return dm


def hand_scan(dm, cfg, meas, poses, pose, seq, t):
    """The branch as a caller composed it before MapBranch: pipeline.py:802-926, :998-1010, step 12b."""
    active = tiling.ma_hex_stencil_tile_ids(CENTER, cfg.H_TILE, cfg.R_ACTIVE_TILES_XY, cfg.R_ACTIVE_TILES_Z)
    stencil = tiling.ma_hex_stencil_tile_ids(CENTER, cfg.H_TILE, cfg.R_STENCIL_TILES_XY, cfg.R_STENCIL_TILES_Z)
    _, _, _, ist = PM.primitive_map_recency_inflate(dm, [dm.dense_tile(k) for k in active], seq,
                                                    cfg.RECENCY_DECAY_LAMBDA, cfg.RECENCY_MIN_SCALE)
    view = extract_atlas_map_view(dm, stencil, cfg.M_TILE_VIEW, cfg.eps_lift, cfg.eps_mass)
    res, _, _ = associate_primitives_ot(meas, view, cfg.association_config(seq))
    Lp, hp, _, _ = visual_pose_evidence_batched(res, meas, view, poses, cfg.eps_lift, cfg.eps_mass)
    stats = dict(staleness_inflation_strength=ist.staleness_inflation_strength,
                 staleness_cov_inflation_trace=ist.staleness_cov_inflation_trace,
                 stale_precision_downscale_total=ist.stale_precision_downscale_total)
    r, _, _ = PM.primitive_map_update_from_association(dm, res, meas, active, pose, t, seq, cfg.map_update,
                                                       map_branch_stats=stats, maintenance="device")
    return Lp, r


def summary(v):
    v = sorted(v)
    return dict(median_ms=statistics.median(v), p10_ms=v[len(v) // 10], p90_ms=v[(9 * len(v)) // 10], n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--m-tile", type=int, default=GC_M_TILE)
    ap.add_argument("--n-valid", type=int, default=4096, help="occupied slots per tile at the start")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _abi.default_context()
    rng = np.random.default_rng(0)
    keys, fields, meas_h = build(rng, a.m_tile, a.n_valid)
    cfg = MapBranchConfig(map_update=PM.MapUpdateConfig(k_insert_tile=GC_K_INSERT_TILE))
    meas = _Obj(**meas_h)
    pose = np.array([0.05, -0.03, 0.0, 0.0, 0.0, 0.04])
    poses = np.stack([pose, pose + 0.01])
    maps = {s: fresh_map(ctx, keys, a.m_tile, a.n_valid, fields) for s in ("branch", "hand")}
    branch = MapBranch(maps["branch"], cfg)
    lines = [f"shape: N = {meas_h['weights'].shape[0]}, H = 2, K = {cfg.k_assoc}, 7 active of {len(keys)} tiles, "
             f"m_tile = {a.m_tile}, M_TILE_VIEW = {cfg.M_TILE_VIEW}, k_insert_tile = {GC_K_INSERT_TILE}, "
             f"{a.n_valid} valid slots per tile at the start",
             f"timing: host wall clock, stream drained before and after each sample; {a.warmup} warm-ups, "
             f"median of {a.iters} [p10-p90]"]
    samples = {"branch": [], "hand": []}
    same = True
    for it in range(a.warmup + a.iters):
        seq, t = 20 + it, 0.1 * it
        out = {}
        for s in ("branch", "hand"):
            ctx.sync()
            t0 = time.perf_counter()
            if s == "branch":
                f = branch.front(meas, CENTER, poses, seq)
                r, _, _ = branch.update(f, pose, t)
                out[s] = (f.L_lidar, r)
            else:
                out[s] = hand_scan(maps[s], cfg, meas, poses, pose, seq, t)
            ctx.sync()
            if it >= a.warmup:
                samples[s].append(1e3 * (time.perf_counter() - t0))
        same = same and out["branch"][0].tobytes() == out["hand"][0].tobytes() and \
            (out["branch"][1].n_fused, out["branch"][1].n_inserted, out["branch"][1].n_culled) == \
            (out["hand"][1].n_fused, out["hand"][1].n_inserted, out["hand"][1].n_culled)
    res = {s: summary(v) for s, v in samples.items()}
    res["evidence_and_counters_equal_every_scan"] = bool(same)
    for s in ("branch", "hand"):
        lines.append(f"per scan, {s:6s}: {res[s]['median_ms']:.3f} ms [{res[s]['p10_ms']:.3f}-{res[s]['p90_ms']:.3f}]")
    lines.append(f"L_lidar bits and the update's counters equal on every scan: {same}")
    del maps, branch

    # ---- residency on 7 slabs: two stencils that share 4 tiles
    s1 = tiling.ma_hex_stencil_tile_ids(CENTER, GC_H_TILE, 1, 0)
    s2 = tiling.ma_hex_stencil_tile_ids(CENTER + np.array([GC_H_TILE, 0.0, 0.0]), GC_H_TILE, 1, 0)
    assert len(set(s1) & set(s2)) == 4 and set(s1 + s2) <= set(keys)
    order = s1 + [k for k in keys if k not in s1]
    perm = [keys.index(k) for k in order]
    f7 = {k: np.concatenate([v[d * a.m_tile:(d + 1) * a.m_tile] for d in perm[:7]]) for k, v in fields.items()}
    dm = fresh_map(ctx, order, a.m_tile, a.n_valid, f7, n_tiles=7)
    swap, hit, hit_sync = [], [], []
    for it in range(a.warmup + a.iters):
        want = s2 if it % 2 == 0 else s1
        ctx.sync()
        t0 = time.perf_counter()
        r = dm.ensure_tiles(want)
        ctx.sync()
        dt = 1e3 * (time.perf_counter() - t0)
        assert len(r.evicted) == 3 and len(r.loaded) + len(r.created) == 3
        t0 = time.perf_counter()
        r = dm.ensure_tiles(want)
        t1 = time.perf_counter()
        ctx.sync()
        t2 = time.perf_counter()
        assert len(r.hits) == 7 and not r.evicted
        if it >= a.warmup:
            swap.append(dt)
            hit.append(1e3 * (t1 - t0))
            hit_sync.append(1e3 * (t2 - t0))
    res["swap3"], res["allhit"], res["allhit_with_sync"] = summary(swap), summary(hit), summary(hit_sync)
    mb = 3 * a.m_tile * dm.image_slot_bytes / 1e6
    lines.append(f"ensure_tiles replacing 3 of 7 tiles ({mb:.1f} MB out and {mb:.1f} MB in, pageable host images): "
                 f"{res['swap3']['median_ms']:.3f} ms [{res['swap3']['p10_ms']:.3f}-{res['swap3']['p90_ms']:.3f}]")
    lines.append(f"ensure_tiles, all 7 keys resident: {1e3 * res['allhit']['median_ms']:.1f} us the call alone "
                 f"[{1e3 * res['allhit']['p10_ms']:.1f}-{1e3 * res['allhit']['p90_ms']:.1f}], "
                 f"{1e3 * res['allhit_with_sync']['median_ms']:.1f} us with a synchronise after it")
    text = "\n".join(lines) + "\n" + json.dumps(res, indent=1) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
