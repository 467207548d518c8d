"""The map branch on the device: the batched recency inflate (gc_primitive_map_recency_inflate_tiles)
against the oracle's per-tile operator and the project's per-tile entry, the candidate statistics
(gc_association_candidate_stats) against the restatement of backend/pipeline.py:879-905, MapBranch.front
against the operators composed by hand, and a trajectory on which a map of 9 slabs has to evict and
reload tiles and must still compute, bit for bit, what a map holding every tile computes."""

import time

import numpy as np
import pytest

from oracle import gc_oracle as O
from test_association import _cmp, _meas
from test_gpu_mapupdate import _EXACT, _Obj, _fresh_map

import mapbranch_restatement as MB
import mapmaint_cases as MM
import mapupdate_cases as MC

RTOL = 1e-10
SEQ, LAM, MIN_SCALE = 45, 0.02, 0.5  # last_supported is in [0, 40): decay in [0.41, 0.89], clipped at 0.5 beyond dt = 34
_ASSOC = ("responsibilities", "candidate_pool_indices", "candidate_tile_ids", "candidate_slots", "row_masses",
          "cost_matrix")


def _bits(fields):
    return {k: np.ascontiguousarray(v).tobytes() for k, v in fields.items()}


def _close(a, b, rtol=1e-12):
    return abs(a - b) <= rtol * max(abs(a), abs(b))


# ----------------------------------------------------------------------------- batched recency inflate
def _keyed_map(ctx, case, packed=True):
    """The case's dense tiles under keys 1000 + 7 d, so that a key is never its own dense index."""
    from gcslam.primitive_map import DevicePrimitiveMap
    dm = DevicePrimitiveMap(len(case["tiles"]), case["m_tile"], ctx=ctx, packed=packed)
    dm.upload(**MM.flat(case))
    dm.set_tile_keys([1000 + 7 * d for d in range(dm.n_tiles)])
    return dm


def _dense_tiles(dm):
    full = dm.download()
    m = dm.m_tile
    return [{f: v[d * m:(d + 1) * m] for f, v in full.items()} for d in range(dm.n_tiles)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", MM.CASES)
def test_gpu_recency_inflate_tiles(ctx, name):
    """The mapmaint_cases tile sets hold the shapes that matter here: tiny_m1 is m_tile = 1; ragged and cap
    list a tile with no valid slot; ragged is 300 slots against 256-thread blocks (two blocks per tile, the
    second ragged); wide is 64 of 70 tiles."""
    from gcslam import primitive_map as PM
    case = MM.build(name)
    active = case["active"]
    keys = [1000 + 7 * d for d in active]
    dm = _keyed_map(ctx, case)
    _, cert, eff, stats = PM.primitive_map_recency_inflate_tiles(dm, keys, SEQ, LAM, MIN_SCALE)
    got = _dense_tiles(dm)
    assert stats.per_tile.shape == (len(active), 3) and cert.exact
    # ---- the oracle's per-tile operator looped over the tiles
    sums = np.zeros(3)
    for a, d in enumerate(active):
        ref, st = O.primitive_map_recency_inflate(case["tiles"][d], SEQ, LAM, MIN_SCALE)
        ref = dict(ref, valid_mask=ref["valid_mask"].astype(np.uint8))
        _cmp(got[d], ref, _EXACT, RTOL)
        assert stats.per_tile[a, 0] == st[0], (d, stats.per_tile[a], st)
        for q in (1, 2):
            assert _close(stats.per_tile[a, q], st[q]), (d, q, stats.per_tile[a], st)
        sums += st
    assert eff.predicted == eff.realized == sums[0]
    assert _close(stats.stale_precision_downscale_total, sums[1]), (stats, sums)
    assert _close(stats.staleness_cov_inflation_trace, sums[2]), (stats, sums)
    assert _close(stats.staleness_inflation_strength, sums[1] / max(sums[0], 1.0))
    # ---- tiles not listed: the bits that were uploaded
    flat = MM.flat(case)
    m = case["m_tile"]
    for d in range(dm.n_tiles):
        if d not in active:
            for f, v in got[d].items():
                assert v.tobytes() == np.ascontiguousarray(flat[f][d * m:(d + 1) * m]).tobytes(), (d, f)
    # ---- the project's per-tile entry: one call per tile on a second map, one call for all on a third
    dm2, dm3 = _keyed_map(ctx, case), _keyed_map(ctx, case)
    for a, d in enumerate(active):
        _, _, e1, s1 = PM.primitive_map_recency_inflate(dm2, [d], SEQ, LAM, MIN_SCALE)
        one = np.array([e1.predicted, s1.stale_precision_downscale_total, s1.staleness_cov_inflation_trace])
        assert stats.per_tile[a].tobytes() == one.tobytes(), (d, stats.per_tile[a], one)
    _, _, e3, s3 = PM.primitive_map_recency_inflate(dm3, active, SEQ, LAM, MIN_SCALE)
    assert (eff.predicted, stats.staleness_inflation_strength, stats.staleness_cov_inflation_trace,
            stats.stale_precision_downscale_total) == \
        (e3.predicted, s3.staleness_inflation_strength, s3.staleness_cov_inflation_trace,
         s3.stale_precision_downscale_total)
    assert _bits(dm.download()) == _bits(dm2.download()) == _bits(dm3.download())


@pytest.mark.gpu
def test_gpu_recency_inflate_tiles_keys_layout_and_errors(ctx):
    """An unknown key is skipped; the per-field layout gives the packed one's bits; no key: nothing
    happens; a stored, non-resident key and a duplicate raise."""
    from gcslam import primitive_map as PM
    case = MM.build("ragged")
    keys = [1000 + 7 * d for d in case["active"]]
    base = _keyed_map(ctx, case)
    _, _, eff0, st0 = PM.primitive_map_recency_inflate_tiles(base, keys, SEQ, LAM, MIN_SCALE)
    based = _bits(base.download())
    dm = _keyed_map(ctx, case)
    _, _, eff, st = PM.primitive_map_recency_inflate_tiles(dm, [keys[0], 999999, keys[1], -5, keys[2]], SEQ, LAM,
                                                           MIN_SCALE)
    assert st.per_tile.tobytes() == st0.per_tile.tobytes() and eff.predicted == eff0.predicted
    assert _bits(dm.download()) == based
    dmf = _keyed_map(ctx, case, packed=False)
    _, _, _, stf = PM.primitive_map_recency_inflate_tiles(dmf, keys, SEQ, LAM, MIN_SCALE)
    assert stf.per_tile.tobytes() == st0.per_tile.tobytes() and _bits(dmf.download()) == based
    # nothing to do
    _, cert, eff, st = PM.primitive_map_recency_inflate_tiles(dm, [999999], SEQ, LAM, MIN_SCALE)
    assert cert.exact and eff.predicted == 0.0 and st.per_tile.shape == (0, 3)
    assert (st.staleness_inflation_strength, st.staleness_cov_inflation_trace) == (0.0, 0.0)
    assert _bits(dm.download()) == based
    with pytest.raises(ValueError, match="duplicate"):
        PM.primitive_map_recency_inflate_tiles(dm, [keys[0], keys[0]], SEQ, LAM, MIN_SCALE)
    # tile keys[0] leaves for the host store: it is known, but not resident
    dm.ensure_tiles([k for k in dm.tile_keys if k != keys[0]])
    r = dm.ensure_tiles([555])
    assert r.evicted == [keys[0]]
    with pytest.raises(ValueError, match="host store"):
        PM.primitive_map_recency_inflate_tiles(dm, keys, SEQ, LAM, MIN_SCALE)


@pytest.mark.gpu
def test_gpu_recency_inflate_tiles_does_not_wait(ctx):
    """Behind a 0.5 s device spin the launch returns at once; the statistics, read after the
    synchronise, are those of the operator."""
    from gcslam import _abi
    from gcslam import primitive_map as PM
    case = MM.build("ragged")
    keys = [1000 + 7 * d for d in case["active"]]
    ref = _keyed_map(ctx, case)
    _, _, _, st0 = PM.primitive_map_recency_inflate_tiles(ref, keys, SEQ, LAM, MIN_SCALE)  # also sizes the scratch
    dm = _keyed_map(ctx, case)
    h_dense = np.asarray(PM._recency_tiles_dense(dm, keys), np.int32)
    d_dense, = _abi.upload_many(ctx, [h_dense], [np.int32])
    d_stats = _abi.DeviceArray(ctx, (len(keys), 3), np.float64)
    ctx.sync()
    _abi.call("gc_test_device_spin", ctx.handle, 0.5, ctx=ctx)
    t0 = time.perf_counter()
    PM._recency_tiles_launch(dm, d_dense, h_dense, SEQ, LAM, MIN_SCALE, d_stats)
    t1 = time.perf_counter()
    ctx.sync()
    t2 = time.perf_counter()
    print(f"launch {t1 - t0:.5f} s, synchronise {t2 - t1:.4f} s")
    assert t1 - t0 < 0.25, t1 - t0
    assert d_stats.download().tobytes() == st0.per_tile.tobytes()
    assert _bits(dm.download()) == _bits(ref.download())


# ----------------------------------------------------------------------------- candidate statistics
def _hand_view(ctx, view_valid):
    from gcslam.association import DeviceMapView
    view = DeviceMapView(ctx, [0], len(view_valid), 3)
    view.arrays["valid_mask"].upload(np.asarray(view_valid, np.uint8))
    return view


def _hand_assoc(case):
    from gcslam.association import PrimitiveAssociationResult
    z = np.zeros(case["pool"].shape)
    return PrimitiveAssociationResult(responsibilities=z, candidate_pool_indices=case["pool"],
                                      candidate_tile_ids=case["tiles"], candidate_slots=z.astype(np.int64),
                                      row_masses=z[:, 0], cost_matrix=z)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MB.CASES))
def test_gpu_candidate_stats_hand_made(ctx, name):
    from gcslam.association import association_candidate_stats
    case = MB.CASES[name]
    got = association_candidate_stats(_hand_assoc(case), _Obj(valid_mask=case["valid_meas"]),
                                      _hand_view(ctx, case["view_valid"]), MB.EPS_MASS)
    assert got == MB.expected(case), (name, got)


@pytest.mark.gpu
def test_gpu_candidate_stats_clamp_and_more_than_one_block(ctx):
    """Pool indices outside the view are clamped into it; 700 rows take three workgroups, with K = 16."""
    from gcslam.association import association_candidate_stats
    c = MB._case([1], [[0, 7, -3]], [[-1, 4, 4]], [1, 0, 1])
    got = association_candidate_stats(_hand_assoc(c), _Obj(valid_mask=c["valid_meas"]), _hand_view(ctx, c["view_valid"]))
    assert got == MB.expected(c) and got[MB.NAMES[1]] == 3.0
    rng = np.random.default_rng(2)
    N, K, V = 700, 16, 90
    c = dict(valid_meas=rng.uniform(0, 1, N) < 0.8, pool=rng.integers(0, V, (N, K)).astype(np.int32),
             tiles=rng.integers(50, 56, (N, K)).astype(np.int64), view_valid=rng.uniform(0, 1, V) < 0.6)
    got = association_candidate_stats(_hand_assoc(c), _Obj(valid_mask=c["valid_meas"]), _hand_view(ctx, c["view_valid"]))
    assert got == MB.expected(c), got
    assert 1.0 < got[MB.NAMES[0]] < 6.0 and got[MB.NAMES[2]] > got[MB.NAMES[1]]


@pytest.mark.gpu
def test_gpu_candidate_stats_of_a_device_association(ctx):
    """The association of the `ragged` map-update case computed on the device, its `.device` arrays read
    in place: the result is the restatement applied to the downloaded association."""
    from gcslam.association import (AssociationConfig, association_candidate_stats, associate_primitives_ot,
                                    extract_atlas_map_view)
    case = MC.build("ragged")
    dm = _fresh_map(ctx, case)
    view = extract_atlas_map_view(dm, case["ids"], case["m_view"])
    meas = _Obj(**case["meas"])
    res, _, _ = associate_primitives_ot(meas, view, AssociationConfig(k_assoc=case["K"], scan_seq=MC.SCAN_SEQ,
                                                                      h_tile=MC.H_TILE))
    assert res.device is not None
    got = association_candidate_stats(res, meas, view)
    want = MB.candidate_stats(case["meas"]["valid_mask"], res.candidate_pool_indices, res.candidate_tile_ids,
                              view.download("valid_mask")["valid_mask"])
    assert got == want, (got, want)
    assert got[MB.NAMES[0]] > 1.0 and got[MB.NAMES[1]] > 1.0  # more than one tile among a row's candidates


# ----------------------------------------------------------------------------- MapBranch
def _branch_config(m_view, k_assoc, k_insert):
    from gcslam.map_branch import MapBranchConfig
    from gcslam.primitive_map import MapUpdateConfig
    return MapBranchConfig(M_TILE_VIEW=m_view, k_assoc=k_assoc, H_TILE=MC.H_TILE,
                           map_update=MapUpdateConfig(k_insert_tile=k_insert, h_tile=MC.H_TILE))


def _same_front(a, b):
    assert a.L_lidar.tobytes() == b.L_lidar.tobytes() and a.h_lidar.tobytes() == b.h_lidar.tobytes()
    assert a.vpe_parts.tobytes() == b.vpe_parts.tobytes() and a.vpe_cert.tobytes() == b.vpe_cert.tobytes()
    for k in _ASSOC:
        assert getattr(a.assoc_result, k).tobytes() == getattr(b.assoc_result, k).tobytes(), k
    assert a.map_branch_stats == b.map_branch_stats and len(a.map_branch_stats) == 6
    assert (a.active_tile_ids, a.stencil_tile_ids) == (b.active_tile_ids, b.stencil_tile_ids)
    assert [c.to_dict() for c in a.certs] == [c.to_dict() for c in b.certs]
    assert a.inflate_stats.per_tile.tobytes() == b.inflate_stats.per_tile.tobytes()
    assert _bits(a.map_view.download()) == _bits(b.map_view.download())


_PLAN = ("insert_indices", "insert_valid", "insert_target_slots", "new_ids")
_SCALARS = ("n_fused", "n_inserted", "n_culled", "n_merged", "fused_mass_total", "insert_mass_total",
            "insert_mass_p95", "evicted_mass_total")
# the two fields of the MapUpdateCert that list the map's own slabs: 2 of 9 on one map, all the others on the other
_SLABS = ("n_inactive_tiles", "tile_ids_inactive")


def _same_update(a, b):
    (ra, ca, ea), (rb, cb, eb) = a, b
    for k in _PLAN:
        assert getattr(ra, k).tobytes() == getattr(rb, k).tobytes(), k
    for k in _SCALARS:
        assert getattr(ra, k) == getattr(rb, k), k
    da, db = ca.to_dict(), cb.to_dict()
    ma, mb = da.pop("map_update"), db.pop("map_update")
    assert da == db
    assert {k: v for k, v in ma.items() if k not in _SLABS} == {k: v for k, v in mb.items() if k not in _SLABS}
    assert ea.to_dict() == eb.to_dict()


@pytest.mark.gpu
def test_gpu_map_branch_front_is_the_composition(ctx):
    """On the `ragged` map-update geometry, front and update equal the existing operators called by hand
    in the reference's order (pipeline.py:802-926, :998-1010, step 12b), the per-tile recency inflate
    among them: the same arithmetic, so the same bits."""
    from gcslam import primitive_map as PM
    from gcslam.association import association_candidate_stats, associate_primitives_ot, extract_atlas_map_view
    from gcslam.map_branch import MapBranch
    from gcslam.ops import visual_pose_evidence_batched
    from gcslam.tiling import ma_hex_stencil_tile_ids
    case = MC.build("ragged")
    cfg = _branch_config(case["m_view"], case["K"], case["k_ins"])
    meas = _Obj(**case["meas"])
    center = np.array([1.0, 0.5, 1.0])  # inside cell (0, 0, 0)
    poses = np.stack([case["pose"], case["pose"] + np.array([0.05, -0.02, 0.01, 0.01, -0.02, 0.03])])
    dm = _fresh_map(ctx, case)
    branch = MapBranch(dm, cfg)
    front = branch.front(meas, center, poses, MC.SCAN_SEQ)
    assert front.active_tile_ids == case["active"] and front.residency.hits == case["active"]
    assert front.residency.evicted == [] and front.L_lidar.shape == (2, 22, 22) and front.h_lidar.shape == (2, 22)
    # ---- by hand on a second map
    dm2 = _fresh_map(ctx, case)
    active = ma_hex_stencil_tile_ids(center, cfg.H_TILE, cfg.R_ACTIVE_TILES_XY, cfg.R_ACTIVE_TILES_Z)
    stencil = ma_hex_stencil_tile_ids(center, cfg.H_TILE, cfg.R_STENCIL_TILES_XY, cfg.R_STENCIL_TILES_Z)
    _, icert, _, istats = PM.primitive_map_recency_inflate(dm2, [dm2.dense_tile(k) for k in active], MC.SCAN_SEQ,
                                                           cfg.RECENCY_DECAY_LAMBDA, cfg.RECENCY_MIN_SCALE)
    view = extract_atlas_map_view(dm2, stencil, cfg.M_TILE_VIEW, cfg.eps_lift, cfg.eps_mass)
    res, acert, _ = associate_primitives_ot(meas, view, cfg.association_config(MC.SCAN_SEQ))
    cand = association_candidate_stats(res, meas, view, cfg.eps_mass)
    Lp, hp, parts, cv = visual_pose_evidence_batched(res, meas, view, poses, cfg.eps_lift, cfg.eps_mass)
    assert front.L_lidar.tobytes() == Lp.tobytes() and front.h_lidar.tobytes() == hp.tobytes()
    assert front.vpe_parts.tobytes() == parts.tobytes() and front.vpe_cert.tobytes() == cv.tobytes()
    for k in _ASSOC:
        assert getattr(front.assoc_result, k).tobytes() == getattr(res, k).tobytes(), k
    want = dict(cand, staleness_inflation_strength=istats.staleness_inflation_strength,
                staleness_cov_inflation_trace=istats.staleness_cov_inflation_trace,
                stale_precision_downscale_total=istats.stale_precision_downscale_total)
    assert front.map_branch_stats == want and want["stale_precision_downscale_total"] > 0.0
    assert [c.to_dict() for c in front.certs] == [icert.to_dict(), acert.to_dict()]
    assert _bits(front.map_view.download()) == _bits(view.download())
    assert _bits(dm.download()) == _bits(dm2.download())
    # ---- step 12b
    up = branch.update(front, case["pose"], MC.TIMESTAMP)
    up2 = PM.primitive_map_update_from_association(dm2, res, meas, active, case["pose"], MC.TIMESTAMP, MC.SCAN_SEQ,
                                                   cfg.map_update, map_branch_stats=want, maintenance="device")
    _same_update(up, up2)
    assert up[1].to_dict() == up2[1].to_dict()
    mu = up[1].map_update
    assert (mu.candidate_tiles_per_meas_mean, mu.candidate_primitives_per_meas_mean,
            mu.candidate_primitives_per_meas_p95) == tuple(cand[k] for k in MB.NAMES)
    assert mu.candidate_primitives_per_meas_mean > 0.0 and up[0].n_fused > 0 and up[0].n_inserted > 0
    assert _bits(dm.download()) == _bits(dm2.download())
    assert (dm.next_global_id, dm.total_count, dm.tile_count) == (dm2.next_global_id, dm2.total_count, dm2.tile_count)
    # the reference's two size-mismatch errors
    from dataclasses import replace
    with pytest.raises(ValueError, match="active tile stencil size mismatch"):
        MapBranch(dm, replace(cfg, N_ACTIVE_TILES=9)).front(meas, center, poses, MC.SCAN_SEQ)
    with pytest.raises(ValueError, match="stencil tile size mismatch"):
        MapBranch(dm, replace(cfg, N_STENCIL_TILES=9)).front(meas, center, poses, MC.SCAN_SEQ)


def _tiles_by_key(dm):
    """Every tile of the map under its key: the resident ones from one download, the others from the store."""
    m = dm.m_tile
    full = dm.download()
    out = {k: {f: v[d * m:(d + 1) * m] for f, v in full.items()} for d, k in enumerate(dm.tile_keys)}
    out.update({k: dm.key_fields(k) for k in dm.stored_keys()})
    return out


N_SCANS, N_ROWS = 8, 96
_XS = [0.2 + 2.5 * i for i in (0, 1, 2, 3, 4, 3, 2, 1)]  # out along x and back, 2.5 m per scan


def _scan(i):
    """Scan i of the trajectory: the centre, 96 measurement rows around it (already near their world
    places, so the near-identity pose below keeps them in the active tiles), two hypothesis poses and z_t."""
    rng = np.random.default_rng(100 + i)
    center = np.array([_XS[i], 0.3, 1.0])
    meas = _meas(rng, N_ROWS, -2.0, 2.0)
    pos = meas["thetas"] / 4.0
    pos[:, :2] += center[:2]
    meas["thetas"] = 4.0 * pos
    meas["colors"] = rng.uniform(-0.1, 1.1, (N_ROWS, 3))
    meas["sources"] = (rng.uniform(0, 1, N_ROWS) < 0.6).astype(np.int32)
    pose = np.concatenate([rng.normal(size=3) * 0.02, rng.normal(size=3) * 0.01])
    pose[2] = abs(pose[2]) * 0.1
    poses = np.stack([pose, pose + rng.normal(size=6) * 0.01])
    return center, meas, poses, pose


@pytest.mark.gpu
def test_gpu_map_branch_trajectory_evicts_reloads_and_matches_a_static_map(ctx):
    """Eight scans, H = 2, 96 rows, m_tile = 64, M_TILE_VIEW = 16, k_assoc = 8, k_insert_tile = 8, through
    a MapBranch on 9 slabs (7 active, so the moving stencil evicts, and the way back reloads) and through
    one on a map that holds every tile of the trajectory from the start. Every scan's evidence,
    association, statistics, update result and certificates, and in the end every tile, are the same
    bits on both."""
    from gcslam.map_branch import MapBranch
    from gcslam.primitive_map import DevicePrimitiveMap
    from gcslam.tiling import ma_hex_stencil_tile_ids
    cfg = _branch_config(16, 8, 8)
    scans = [_scan(i) for i in range(N_SCANS)]
    every = list(dict.fromkeys(k for c, _, _, _ in scans for k in ma_hex_stencil_tile_ids(c, MC.H_TILE, 1, 0)))
    assert len(every) > 9
    small = DevicePrimitiveMap(9, 64, ctx=ctx)
    big = DevicePrimitiveMap(len(every), 64, ctx=ctx)
    big.set_tile_keys(every)
    b_small, b_big = MapBranch(small, cfg), MapBranch(big, cfg)
    evicted, reloaded = set(), set()
    insert_on_reloaded = fuse_on_reloaded = 0
    for i, (center, meas, poses, pose) in enumerate(scans):
        f1 = b_small.front(_Obj(**meas), center, poses, i + 1)
        f2 = b_big.front(_Obj(**meas), center, poses, i + 1)
        assert f2.residency.hits == f2.active_tile_ids and not f2.residency.evicted, i
        _same_front(f1, f2)
        evicted |= {k for k in f1.residency.evicted if k in every}
        reloaded |= set(f1.residency.loaded)
        assert set(f1.residency.loaded) <= evicted, i
        u1 = b_small.update(f1, pose, 0.1 * (i + 1))
        u2 = b_big.update(f2, pose, 0.1 * (i + 1))
        _same_update(u1, u2)
        # what happened on the tiles that came back from the store in this scan
        back = [a for a, k in enumerate(f1.active_tile_ids) if k in f1.residency.loaded]
        insert_on_reloaded += int(sum((u1[0].new_ids[a] >= 0).sum() for a in back))
        a_res = f1.assoc_result
        hit = np.isin(a_res.candidate_tile_ids, [f1.active_tile_ids[a] for a in back]) & \
            (a_res.responsibilities > 0.0) & np.asarray(meas["valid_mask"], bool)[:, None]
        fuse_on_reloaded += int(hit.sum())
        print(f"scan {i}: x = {center[0]:.1f}, loaded {len(f1.residency.loaded)}, created "
              f"{len(f1.residency.created)}, evicted {len(f1.residency.evicted)}, fused {u1[0].n_fused}, "
              f"inserted {u1[0].n_inserted}, merged {u1[0].n_merged}, culled {u1[0].n_culled}")
    # the run means something only if tiles left, came back, and were written after coming back
    assert evicted and reloaded, (evicted, reloaded)
    assert insert_on_reloaded > 0 and fuse_on_reloaded > 0, (insert_on_reloaded, fuse_on_reloaded)
    # ---- the maps in the end, tile by tile under their keys (resident or stored)
    assert (small.next_global_id, small.total_count) == (big.next_global_id, big.total_count)
    assert small.next_global_id > 0
    assert set(small.tile_keys + small.stored_keys()) >= set(every) and small.stored_keys()
    t_small, t_big = _tiles_by_key(small), _tiles_by_key(big)
    for k in every:
        assert _bits(t_small[k]) == _bits(t_big[k]), k
        assert small.key_count(k) == big.key_count(k), k
        d = small.dense_tile(k)
        cc = small._tile_cc[d] if d >= 0 else small._store[k].colors_current
        assert cc == big._tile_cc[big.dense_tile(k)], k
