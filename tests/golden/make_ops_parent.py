"""TEST INFRASTRUCTURE — records what the operators outside the hot path computed before their
fixed-order sums moved into csrc/gc_blocksum.h and their scratch layouts onto the carver of
gc_internal.h, for the bit-identity check of tests/test_gpu_ops_parent_bits.py. Run on an MI355X with
the library built from the commit BEFORE that change:

    python tests/golden/make_ops_parent.py

  ops_parent.npz   "<group>/<case>/<array>" for the groups below. None of these grids follows the
                   compute-unit count, so the arrays do not depend on the device.

    vpe        visual_pose_evidence_batched on every vpe_cases case (multi_wg: 10 collapse workgroups,
               more than the 8 chains of the second pass): L_pose, h_pose, parts, cert.
    surfel     extract_lidar_surfels on surfel_cases smoke and overflow_truncate, and on wide_centre
               below (16,647 points: 66 centre workgroups, more than the 64 chains of the centre's
               second pass): the nine batch arrays, the slot cells, n_lidar_valid.
    camsplat   camera_measurement_batch(return_diag=True) on every camsplat_cases case: the
               evidence / fusion arrays and the nine batch arrays.
    assoc      associate_primitives_ot on the map of test_association.py with N = 1,100 rows (the
               1024-thread Sinkhorn's strided loops run twice) and K = 8 of 16 compiled columns:
               responsibilities, row masses, the certificate values.
    mapops     recency -> cull(max_primitives) -> insert_masked -> merge_reduce of test_map_ops.py on
               a 600-slot tile (three reduction workgroups): every returned statistic, the tile after.
    mapupdate  primitive_map_update_from_association (maintenance on) on every mapupdate_cases case:
               the plan, the counters and masses, the active tiles after.

The inputs are rebuilt from seeds by the case modules and the functions below (the test imports them),
so the file holds outputs only. Nothing here computes a reference: the arrays are the library's own, bit
for bit. An array that holds NaN by contract (a query without LiDAR evidence) is stored with the NaNs
zeroed next to their mask ("<array>__nan"), so that every stored array is finite and np.array_equal can
hold.
"""

from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (TESTS, os.path.join(ROOT, "fl-slam_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "ops_parent.npz")
WIDE_CENTRE_N = 16647  # 66 workgroups of 256 points
ASSOC_N, ASSOC_K = 1100, 8
MAPOPS_M = 600


class _Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _put(out, name, a):
    a = np.asarray(a)
    if a.dtype.kind == "f" and np.isnan(a).any():
        out[name + "__nan"] = np.isnan(a)
        a = np.where(np.isnan(a), 0.0, a)
    out[name] = a


def _put_batch(out, pre, batch):
    from gcslam.measurement_batch import BATCH_ARRAYS
    for k in BATCH_ARRAYS:
        _put(out, pre + k, getattr(batch, k))


def run_vpe(ctx):
    from gcslam.association import PrimitiveAssociationResult, extract_atlas_map_view
    from gcslam.ops import visual_pose_evidence_batched
    from test_association import _device_map
    import vpe_cases as VC
    out = {}
    for name in VC.CASES:
        case = VC.build(name)
        dm = _device_map(ctx, case["tiles"], case["m_tile"])
        view = extract_atlas_map_view(dm, case["ids"], case["m_view"])
        a = case["assoc"]
        z = np.zeros(a["responsibilities"].shape, np.int64)
        assoc = PrimitiveAssociationResult(a["responsibilities"], a["candidate_pool_indices"], z, z, a["row_masses"],
                                           np.zeros(a["responsibilities"].shape))
        Lp, hp, parts, cv = visual_pose_evidence_batched(assoc, _Obj(**case["meas"]), view, case["poses"])
        for k, v in (("L_pose", Lp), ("h_pose", hp), ("parts", parts), ("cert", cv)):
            _put(out, f"vpe/{name}/{k}", v)
    return out


def surfel_inputs(name):
    import surfel_cases as SC
    if name == "wide_centre":
        p, t, w = SC.scene(WIDE_CENTRE_N, 0)
        return dict(points=p, timestamps=t, weights=w, cfg=dict(SC._SMALL))
    return SC.build(name)


def run_surfel(ctx):
    from gcslam.ops import SurfelExtractionConfig, extract_lidar_surfels
    out = {}
    for name in ("smoke", "overflow_truncate", "wide_centre"):
        c = surfel_inputs(name)
        batch, _, _ = extract_lidar_surfels(c["points"], c["timestamps"], c["weights"],
                                            SurfelExtractionConfig(**c["cfg"]), ctx=ctx)
        _put_batch(out, f"surfel/{name}/", batch)
        _put(out, f"surfel/{name}/lidar_slot_cells", batch.lidar_slot_cells)
        _put(out, f"surfel/{name}/n_lidar_valid", batch.n_lidar_valid)
    return out


def run_camsplat(ctx):
    import camsplat_cases as CC
    from gcslam.ops import CameraFeatures, PinholeIntrinsics, camera_measurement_batch
    g = np.load(CC.GOLDEN)
    out = {}
    for name in CC.CASES:
        c = CC.load(name, g)
        batch, diag = camera_measurement_batch(c["points_base"], CameraFeatures(**c["features"]),
                                               PinholeIntrinsics(CC.FX, CC.FY, CC.CX, CC.CY), CC.R_BASE_CAMERA,
                                               CC.T_BASE_CAMERA, CC.TIMESTAMP, CC.config(c), n_feat=c["n_feat"],
                                               n_surfel=c["n_surfel"], eps_lift=CC.EPS_LIFT, ctx=ctx, return_diag=True)
        for k in diag.__dataclass_fields__:
            _put(out, f"camsplat/{name}/diag_{k}", getattr(diag, k))
        _put_batch(out, f"camsplat/{name}/", batch)
        _put(out, f"camsplat/{name}/n_camera_valid", batch.n_camera_valid)
    return out


def run_assoc(ctx):
    """The case of test_association.py test_gpu_association_matches_oracle (uniform masses) with more rows."""
    from gcslam.association import AssociationConfig, associate_primitives_ot, extract_atlas_map_view
    from test_association import _device_map, _hex_map, _meas
    rng = np.random.default_rng(5)
    tiles = _hex_map(rng, 64, 60, [(a, b, 0) for a in range(-2, 3) for b in range(-2, 3)])
    view = extract_atlas_map_view(_device_map(ctx, tiles, 64), list(tiles), 32)
    res, cert, eff = associate_primitives_ot(_Obj(**_meas(rng, ASSOC_N)), view,
                                             AssociationConfig(k_assoc=ASSOC_K, scan_seq=9))
    ot = cert.ot
    out = {}
    _put(out, "assoc/responsibilities", res.responsibilities)
    _put(out, "assoc/row_masses", res.row_masses)
    _put(out, "assoc/cert", np.array([ot.marginal_defect_a, ot.marginal_defect_b, ot.transport_mass_total, ot.sum_a,
                                      ot.sum_b, ot.sum_m, ot.sum_novel, cert.support.ess_total, ot.nonzero_a,
                                      ot.nonzero_b, eff.realized], np.float64))
    return out


def run_mapops(ctx):
    """The maintenance sequence of test_map_ops.py on tile 1 of a 3-tile packed map of MAPOPS_M slots."""
    from gcslam import primitive_map as PM
    from test_map_ops import L, _random_tile, _upload
    rng = np.random.default_rng(42)
    M = MAPOPS_M
    dm = PM.DevicePrimitiveMap(3, M, ctx=ctx, packed=True)
    for t_id in range(3):
        _upload(dm, t_id, _random_tile(rng, M))
    out = {}
    _, _, eff, st = PM.primitive_map_recency_inflate(dm, [1], 37, 0.02, 0.05)
    _put(out, "mapops/recency", np.array([eff.realized, st.stale_precision_downscale_total,
                                          st.staleness_cov_inflation_trace, st.staleness_inflation_strength]))
    res, _, _ = PM.primitive_map_cull(dm, 1, 1e-3, max_primitives=M // 2)
    _put(out, "mapops/cull", np.array([res.n_culled, res.mass_dropped], np.float64))
    K = 64
    mask = rng.uniform(0, 1, K) < 0.8
    B = rng.normal(size=(K, 3, 3))
    dm.next_global_id = 1000
    res, _, _ = PM.primitive_map_insert_masked(dm, 1, B @ np.swapaxes(B, 1, 2) + np.eye(3), rng.normal(size=(K, 3)),
                                               rng.normal(size=(K, L, 3)), rng.uniform(0.1, 1, K), 4.5, mask,
                                               scan_seq=38, colors_new=rng.uniform(-0.1, 1.1, (K, 3)),
                                               sources_new=rng.integers(0, 2, K))
    _put(out, "mapops/insert_counts", np.array([res.n_inserted, dm.tile_count[1]], np.int64))
    _put(out, "mapops/insert_new_ids", res.new_ids)
    _put(out, "mapops/insert_target_slots", res.target_slots)
    res, _, _ = PM.primitive_map_merge_reduce(dm, 1, merge_threshold=2.0, max_pairs=16)
    _put(out, "mapops/merge_counts", np.array([res.n_merged, dm.tile_count[1]], np.int64))
    for k, v in dm.download_tile(1).items():
        _put(out, "mapops/tile_" + k, v)
    return out


def run_mapupdate(ctx):
    from gcslam.association import PrimitiveAssociationResult
    from gcslam.primitive_map import MapUpdateConfig, primitive_map_update_from_association
    from test_association import _device_map
    import mapupdate_cases as MC
    out = {}
    for name in MC.CASES:
        case = MC.build(name)
        dm = _device_map(ctx, case["tiles"], case["m_tile"])
        dm.next_global_id = MC.NEXT_ID
        for d, k in enumerate(dm.tile_keys):
            dm.tile_count[d] = int(case["tiles"][k]["valid_mask"].sum()) if k in case["tiles"] else 0
        dm.total_count = sum(dm.tile_count.values())
        assoc = PrimitiveAssociationResult(**{k: case["assoc"][k] for k in (
            "responsibilities", "candidate_pool_indices", "candidate_tile_ids", "candidate_slots", "row_masses",
            "cost_matrix")})
        res, _, _ = primitive_map_update_from_association(dm, assoc, _Obj(**case["meas"]), case["active"], case["pose"],
                                                          MC.TIMESTAMP, MC.SCAN_SEQ, MapUpdateConfig(**case["cfg"]),
                                                          maintenance=True)
        pre = f"mapupdate/{name}/"
        for k in ("insert_indices", "insert_valid", "insert_target_slots", "new_ids"):
            _put(out, pre + k, getattr(res, k))
        _put(out, pre + "counts", np.array([res.n_fused, res.n_inserted, res.n_culled, res.n_merged], np.int64))
        _put(out, pre + "masses", np.array([res.fused_mass_total, res.insert_mass_total, res.insert_mass_p95,
                                            res.evicted_mass_total], np.float64))
        m = dm.m_tile
        rows = np.concatenate([np.arange(d * m, (d + 1) * m) for d, k in enumerate(dm.tile_keys) if k in case["active"]])
        for k, v in dm.download().items():
            _put(out, pre + "map_" + k, v[rows])
    return out


GROUPS = dict(vpe=run_vpe, surfel=run_surfel, camsplat=run_camsplat, assoc=run_assoc, mapops=run_mapops,
              mapupdate=run_mapupdate)


def main():
    from gcslam import _abi
    ctx = _abi.default_context()
    out = {}
    for name, run in GROUPS.items():
        got = run(ctx)
        assert got and all(k.startswith(name + "/") for k in got), name
        out.update(got)
    for k, v in out.items():
        assert np.all(np.isfinite(v.astype(np.float64))), k  # np.array_equal must be able to hold
    np.savez_compressed(OUT, **out)
    print(len(out), "arrays,", os.path.getsize(OUT), "bytes")
    for k, v in out.items():
        print(k, v.dtype, v.shape)


if __name__ == "__main__":
    main()
