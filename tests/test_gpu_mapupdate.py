"""primitive_map_update_from_association on the device (gc_mapupdate.hip) against the NumPy
restatement of the reference's step 12b (tests/mapupdate_restatement.py; "parity unpinned" against
reference outputs) and against the project's own per-tile drop-ins looped on a second device map
(tests/mapupdate_dropins.py). Discrete outputs (plan indices, masks, target slots, new ids,
valid_mask, primitive_ids, the scan-seq fields, timestamps, the integer counters) must be equal;
every float field of every tile, active or not, meets the 1e-10 bar of the surfel and VPE tests
(_cmp: relative to the array's max-abs). The cases' margins (test_mapupdate.py) make the discrete
comparison well posed."""

import numpy as np
import pytest

from oracle import gc_oracle as O
from test_association import _cmp, _device_map, _hex_map

import mapupdate_cases as MC
import mapupdate_dropins as MD

RTOL = 1e-10
_EXACT = ("valid_mask", "primitive_ids", "last_supported_scan_seq", "last_update_scan_seq", "timestamps")
_PLAN = ("insert_indices", "insert_valid", "insert_target_slots", "new_ids")
_COUNTS = ("n_fused", "n_inserted", "n_culled", "n_merged")
_MASSES = ("fused_mass_total", "insert_mass_total", "insert_mass_p95", "evicted_mass_total")


class _Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _fresh_map(ctx, case):
    dm = _device_map(ctx, case["tiles"], case["m_tile"])  # plus one unlisted dense tile (key -1)
    dm.next_global_id = MC.NEXT_ID
    for d, k in enumerate(dm.tile_keys):
        dm.tile_count[d] = int(case["tiles"][k]["valid_mask"].sum()) if k in case["tiles"] else 0
    dm.total_count = sum(dm.tile_count.values())
    return dm


def _assoc(case, **over):
    from gcslam.association import PrimitiveAssociationResult
    a = dict(case["assoc"], **over)
    return PrimitiveAssociationResult(**{k: a[k] for k in ("responsibilities", "candidate_pool_indices",
                                                           "candidate_tile_ids", "candidate_slots", "row_masses",
                                                           "cost_matrix")})


def _update(ctx, case, maintenance, dm=None, assoc=None, batch=None, **kw):
    from gcslam.primitive_map import MapUpdateConfig, primitive_map_update_from_association
    dm = dm or _fresh_map(ctx, case)
    out = primitive_map_update_from_association(dm, assoc or _assoc(case), batch or _Obj(**case["meas"]),
                                                case["active"], case["pose"], MC.TIMESTAMP, MC.SCAN_SEQ,
                                                MapUpdateConfig(**case["cfg"]), maintenance=maintenance, **kw)
    return dm, out


def _tiles_of(dm):
    full = dm.download()
    full["valid_mask"] = full["valid_mask"].astype(bool)
    m = dm.m_tile
    return {k: {f: v[d * m:(d + 1) * m] for f, v in full.items()} for d, k in enumerate(dm.tile_keys)}


def _check_map(got, ref_tiles, m_tile):
    for key, t in got.items():
        ref = ref_tiles.get(key, O.empty_tile(m_tile))  # the unlisted dense tile stays empty
        _cmp(t, ref, _EXACT, RTOL)


def _check_result(res, ref):
    for k in _PLAN:
        np.testing.assert_array_equal(getattr(res, k) if not isinstance(res, dict) else res[k], ref[k], err_msg=k)
    for k in _COUNTS:
        assert (getattr(res, k) if not isinstance(res, dict) else res[k]) == ref[k], k
    for k in _MASSES:
        g = getattr(res, k) if not isinstance(res, dict) else res[k]
        assert abs(g - ref[k]) <= RTOL * max(1.0, abs(ref[k])), (k, g, ref[k])


@pytest.mark.gpu
@pytest.mark.parametrize("maintenance", [False, True])
@pytest.mark.parametrize("name", list(MC.CASES))
def test_gpu_map_update_matches_restatement(ctx, name, maintenance):
    case = MC.build(name)
    ref = MC.reference(case, maintenance)
    MC.check_margins(ref)
    dm, (res, cert, eff) = _update(ctx, case, maintenance)
    _check_result(res, ref)
    _check_map(_tiles_of(dm), ref["tiles"], case["m_tile"])
    # host bookkeeping, from the one download
    assert dm.next_global_id == ref["next_global_id"]
    for d, k in enumerate(dm.tile_keys):
        if k in case["active"]:
            assert dm.tile_count[d] == int(ref["tiles"][k]["valid_mask"].sum()), k
    # certificate and effect (pipeline.py:1454-1487)
    mu = cert.map_update
    A = len(case["active"])
    assert cert.exact and cert.anchor_id == "map_update" and mu.n_active_tiles == A
    assert mu.tile_ids_active == case["active"] and mu.tile_cache_hits == A and mu.tile_cache_misses == 0
    assert mu.tile_ids_inactive == [k for k in dm.tile_keys if k not in case["active"]]
    assert mu.n_inactive_tiles == len(dm.tile_keys) - A
    assert (mu.fused_count, mu.insert_count_total, mu.evicted_count, mu.merged_count) == tuple(ref[k] for k in _COUNTS)
    assert (mu.fused_mass_total, mu.insert_mass_total, mu.insert_mass_p95, mu.evicted_mass_total) == \
        (res.fused_mass_total, res.insert_mass_total, res.insert_mass_p95, res.evicted_mass_total)
    assert eff.objective_name == "primitive_map_update" and eff.predicted == A * case["k_ins"]
    assert eff.realized == res.n_inserted
    assert res.insert_mass_p95 == ref["insert_mass_p95"]  # a selected element, not a sum


@pytest.mark.gpu
@pytest.mark.parametrize("maintenance", [False, True])
@pytest.mark.parametrize("name", ["ragged", "blocks"])
def test_gpu_map_update_matches_dropins(ctx, name, maintenance):
    case = MC.build(name)
    dm, (res, _, _) = _update(ctx, case, maintenance)
    dm2 = _fresh_map(ctx, case)
    ref = MD.dropin_map_update(dm2, case["assoc"], case["meas"], case["active"], case["pose"], MC.TIMESTAMP,
                               MC.SCAN_SEQ, case["cfg"], maintenance)
    _check_result(res, ref)
    _check_map(_tiles_of(dm), _tiles_of(dm2), case["m_tile"])
    assert (dm.next_global_id, dm.total_count, dm.tile_count) == (dm2.next_global_id, dm2.total_count, dm2.tile_count)
    assert dm._tile_cc == dm2._tile_cc


def _same_bits(a, b):
    (dma, (ra, ca, ea)), (dmb, (rb, cb, eb)) = a, b
    fa, fb = dma.download(), dmb.download()
    for k in fa:
        assert fa[k].tobytes() == fb[k].tobytes(), k
    for k in _PLAN:
        assert getattr(ra, k).tobytes() == getattr(rb, k).tobytes(), k
    for k in _COUNTS + _MASSES:
        assert getattr(ra, k) == getattr(rb, k), k
    assert ca.to_dict() == cb.to_dict() and ea.realized == eb.realized
    assert (dma.next_global_id, dma.total_count) == (dmb.next_global_id, dmb.total_count)
    assert dma.tile_count == dmb.tile_count


@pytest.mark.gpu
def test_gpu_map_update_two_runs_bitwise(ctx):
    case = MC.build("ragged")
    _same_bits(_update(ctx, case, True), _update(ctx, case, True))


@pytest.mark.gpu
def test_gpu_map_update_device_inputs_bitwise(ctx):
    """The association's and the batch's `.device` arrays are read in place: the same bits as from host
    arrays, with the host copies poisoned."""
    from gcslam import _abi
    from gcslam.measurement_batch import BATCH_ARRAYS, MeasurementBatch
    case = MC.build("ragged")
    N = case["N"]
    host = _update(ctx, case, True)
    adev = {k: _abi.DeviceArray.from_host(ctx, v, v.dtype) for k, v in case["assoc"].items()}
    poisoned = {k: np.full_like(v, -7 if v.dtype.kind == "i" else np.nan) for k, v in case["assoc"].items()}
    assoc = _assoc(dict(assoc=poisoned))
    assoc.device = adev
    m = dict(case["meas"], source_indices=np.arange(N, dtype=np.int32), timestamps=np.zeros(N))
    mdev = {k: _abi.DeviceArray.from_host(ctx, np.ascontiguousarray(m[k]).astype(dt), dt)
            for k, (_, _, dt) in BATCH_ARRAYS.items()}
    batch = MeasurementBatch(**{k: np.full(np.shape(m[k]), np.nan) for k in BATCH_ARRAYS}, n_feat=0, n_surfel=N,
                             n_camera_valid=0, n_lidar_valid=int(case["meas"]["valid_mask"].sum()), device=mdev)
    dev = _update(ctx, case, True, assoc=assoc, batch=batch)
    _same_bits(host, dev)


@pytest.mark.gpu
def test_gpu_map_update_event_log(ctx):
    case = MC.build("blocks")
    ref = MC.reference(case, False)
    _, (res, _, _) = _update(ctx, case, False, event_log=True)
    ent = res.event_log_entries
    A, k = len(case["active"]), case["k_ins"]
    assert len(ent) == A * k  # every tile inserted something: all of its proposals are logged
    w = np.asarray([e["weight"] for e in ent]).reshape(A, k)
    for a, t in enumerate(case["active"]):
        idx = ref["insert_indices"][a]
        in_tile = ref["meas_tile_ids"][idx] == t
        want = np.where(in_tile, ref["novelty"][idx] * case["meas"]["weights"][idx], 0.0)
        np.testing.assert_array_equal(w[a], want)
        assert all(e["tile_id"] == t and e["timestamp"] == MC.TIMESTAMP for e in ent[a * k:(a + 1) * k])
        Lw, tw, _ = O.transform_gaussian_to_world(case["meas"]["Lambdas"][idx], case["meas"]["thetas"][idx],
                                                  case["meas"]["etas"][idx], case["pose"])
        mu = np.linalg.solve(Lw + O.EPS_LIFT * np.eye(3)[None], tw[..., None])[..., 0]
        _cmp(dict(mu=np.asarray([e["mu_world"] for e in ent[a * k:(a + 1) * k]])), dict(mu=mu), (), RTOL)
        np.testing.assert_array_equal(np.asarray([e["color"] for e in ent[a * k:(a + 1) * k]]),
                                      case["meas"]["colors"][idx])


@pytest.mark.gpu
def test_gpu_map_update_device_chain_two_scans(ctx):
    """surfels -> view -> association -> update on one map, all through `.device`, for two consecutive
    scans: the host bookkeeping equals a recount of the downloaded map after each, and the second
    scan's association sees the primitives the first one inserted."""
    from gcslam.association import AssociationConfig, associate_primitives_ot, extract_atlas_map_view
    from gcslam.ops import SurfelExtractionConfig, extract_lidar_surfels
    from gcslam.primitive_map import MapUpdateConfig, primitive_map_update_from_association
    import surfel_cases as SC
    rng = np.random.default_rng(13)
    cells = [(a, b, cz) for a in range(-1, 1) for b in range(-1, 1) for cz in (-1, 0)]
    tiles = _hex_map(rng, 96, 60, cells)  # room for both scans' inserts: no live slot is evicted
    dm = _device_map(ctx, tiles, 96)
    keys = list(tiles)
    for d, k in enumerate(dm.tile_keys):
        dm.tile_count[d] = int(tiles[k]["valid_mask"].sum()) if k in tiles else 0
    dm.total_count = sum(dm.tile_count.values())
    dm.next_global_id = 5000
    c = SC.build("overflow_truncate")
    scfg = SurfelExtractionConfig(**c["cfg"])
    cfg = MapUpdateConfig(k_insert_tile=8, block_size=32)
    pose = np.array([0.02, -0.01, 0.03, 0.01, -0.02, 0.015])
    seen_new = False
    for scan in range(2):
        seq = 20 + scan
        pts = c["points"] + (0.0 if scan == 0 else 0.004)
        batch, _, _ = extract_lidar_surfels(pts, c["timestamps"], c["weights"], scfg, ctx=ctx, device_out=True)
        view = extract_atlas_map_view(dm, keys, 96)
        assoc, _, _ = associate_primitives_ot(batch, view, AssociationConfig(scan_seq=seq))
        assert assoc.device is not None and batch.device is not None
        if scan == 1:  # the view of the updated map offers the first scan's inserts as candidates
            vids = view.download("primitive_ids", "valid_mask")
            seen_new = bool(np.any(vids["primitive_ids"][vids["valid_mask"]] >= 5000))
        before = dm.next_global_id
        # the first scan keeps its zero-mass inserts (no cull), so the second one's view can show them
        res, cert, _ = primitive_map_update_from_association(dm, assoc, batch, keys, pose, 3.0 + scan, seq, cfg,
                                                             maintenance=scan == 1)
        got = dm.download("valid_mask", "primitive_ids")
        vm = got["valid_mask"].astype(bool)
        for d in range(dm.n_tiles):
            assert dm.tile_count.get(d, 0) == int(vm[d * 96:(d + 1) * 96].sum()), d
        assert dm.total_count == int(vm.sum())
        assert dm.next_global_id == before + res.n_inserted
        new = res.new_ids[res.insert_valid]
        assert np.array_equal(new, before + np.arange(res.n_inserted)) and res.n_inserted >= len(keys)
        alive = got["primitive_ids"][vm]
        assert alive.max() < dm.next_global_id and np.unique(alive[alive >= 5000]).shape[0] == (alive >= 5000).sum()
        assert res.n_fused > 0 and res.fused_mass_total > 0.0 and cert.map_update.fused_count == res.n_fused
    assert seen_new
