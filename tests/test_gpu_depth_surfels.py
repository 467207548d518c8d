"""RGB-D surfel extraction on the device (gc_depthsurfel.hip, gcslam/ops/depth_surfel_extraction.py) against
its NumPy restatement (tests/depth_surfel_restatement.py; the operator is this build's, so the restatement is
what pins it). The cases and the preconditions asserted on the restatement alone are in
tests/depth_surfel_cases.py. Floating-point outputs are compared at 1e-10 relative to the array's max-abs (the
_cmp convention of test_association.py, the bar the LiDAR extractor meets against the same fit); counts,
masks, sources, indices and the slot -> cell record exactly.

As in test_gpu_surfels.py, Lambdas, thetas, etas and the grey of `no_rgb` are compared on the
orientation-determined slots; weights, timestamps, colours and the position solve(Λ + eps_lift I, θ) on every
valid slot."""

import numpy as np
import pytest

from gcslam import _abi
from gcslam.certificates import InfluenceCert
from gcslam.measurement_batch import BATCH_ARRAYS
from gcslam.ops import DepthSurfelConfig, MeasurementBatch, PinholeIntrinsics, extract_depth_surfels
from oracle import gc_oracle as O
from test_association import _cmp

import depth_surfel_cases as DC

pytestmark = pytest.mark.gpu

RTOL = 1e-10
TRIGGERS = ["depth_cell_binning", "plane_fit_batched", "wishart_regularization"]
PARITY = ("planes", "edge", "overflow", "no_rgb", "quadratic")


class _Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _base(name, ctx=None):
    """The case's base batch (None without one): host-resident, or with ctx on the device."""
    c = DC.build(name)
    if c["base"] is None:
        return None
    cfg = DepthSurfelConfig(**c["cfg"])
    b = DC.base_arrays(cfg.n_feat, cfg.n_surfel, c["base"])
    arrays = {k: np.array(b[k]) for k in BATCH_ARRAYS}
    counts = dict(n_feat=cfg.n_feat, n_surfel=cfg.n_surfel, n_camera_valid=b["n_camera_valid"], n_lidar_valid=b["n_lidar_valid"])
    if ctx is None:
        return MeasurementBatch(**arrays, **counts)
    dev = {k: _abi.DeviceArray.from_host(ctx, arrays[k], BATCH_ARRAYS[k][2]) for k in BATCH_ARRAYS}
    return MeasurementBatch(**dev, **counts, device=dev)


def _run(ctx, name, base="case", **kw):
    c = DC.build(name)
    return extract_depth_surfels(c["depth"], c["rgb"], PinholeIntrinsics(*c["K"]), c["R"], c["t"], c["timestamp"],
                                 DepthSurfelConfig(**c["cfg"]), base_batch=_base(name) if base == "case" else base,
                                 ctx=ctx, **kw)


def _same(a: MeasurementBatch, b: MeasurementBatch):
    for k in BATCH_ARRAYS:
        x, y = np.asarray(getattr(a, k)), np.asarray(getattr(b, k))
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert (a.n_feat, a.n_surfel, a.n_camera_valid, a.n_lidar_valid) == (b.n_feat, b.n_surfel, b.n_camera_valid,
                                                                         b.n_lidar_valid)
    np.testing.assert_array_equal(np.asarray(a.depth_slot_cells), np.asarray(b.depth_slot_cells))


def _check_cert(cert, eff, n_new, free, anchor="depth_surfel_extraction"):
    assert not cert.exact and cert.approximation_triggers == TRIGGERS and not cert.frobenius_applied
    assert cert.chart_id == "GC-RIGHT-01" and cert.anchor_id == anchor
    assert cert.support.ess_total == float(n_new) and cert.support.support_frac == n_new / max(free, 1)
    assert cert.influence == InfluenceCert.identity()
    assert eff.objective_name == "depth_surfel_extraction" and eff.predicted == eff.realized == float(n_new)


@pytest.mark.parametrize("name", PARITY)
def test_gpu_depth_surfels_match_restatement(ctx, name):
    ref = DC.reference(name)
    DC.check_conditions(ref)
    batch, cert, eff = _run(ctx, name)
    nf, ns, n_in, n_new = ref["n_feat"], ref["n_surfel"], ref["n_in"], ref["n_new"]
    assert isinstance(batch, MeasurementBatch) and batch.device is None and n_new > 0
    assert (batch.n_feat, batch.n_surfel, batch.n_camera_valid, batch.n_lidar_valid) == (nf, ns, n_in + n_new,
                                                                                         ref["n_lidar_valid"])
    for k, (shp, dt, _) in BATCH_ARRAYS.items():
        a = getattr(batch, k)
        assert a.shape == (nf + ns,) + shp and a.dtype == dt, k
    # exact: the mask, the sources, the indices, which cell every row came from
    _cmp(batch.__dict__, {k: ref[k] for k in ("valid_mask", "sources", "source_indices")},
         ("valid_mask", "sources", "source_indices"), 0.0)
    assert batch.depth_slot_cells.shape == (nf,) and batch.depth_slot_cells.dtype == np.int32
    np.testing.assert_array_equal(batch.depth_slot_cells, ref["slot_cells"])
    rows = ref["rows"]
    assert rows.tolist() == list(range(n_in, n_in + n_new))
    # every valid slot: weight, timestamp, colour (the grey depends on the normal), position
    every = ("weights", "timestamps") + (() if name == "no_rgb" else ("colors",))
    _cmp({k: getattr(batch, k)[rows] for k in every}, {k: ref[k][rows] for k in every}, (), RTOL)
    assert (batch.timestamps[rows] == DC.build(name)["timestamp"]).all()
    pos = np.linalg.solve(batch.Lambdas[rows] + O.EPS_LIFT * np.eye(3)[None], batch.thetas[rows][..., None])[..., 0]
    ref_pos = np.linalg.solve(ref["Lambdas"][rows] + O.EPS_LIFT * np.eye(3)[None], ref["thetas"][rows][..., None])[..., 0]
    _cmp(dict(positions=pos), dict(positions=ref_pos), (), RTOL)
    # orientation-determined slots: everything that depends on the normal
    det = ref["slot_determined"]
    assert det.sum() >= 0.9 * n_new
    normal_fields = ("Lambdas", "thetas", "etas") + (("colors",) if name == "no_rgb" else ())
    _cmp({k: getattr(batch, k)[rows][det] for k in normal_fields}, {k: ref[k][rows][det] for k in normal_fields}, (), RTOL)
    assert not batch.etas[rows, 1:].any()
    # every other row is the base batch's (zeros without one), bitwise
    base = _base(name)
    other = np.setdiff1d(np.arange(nf + ns), rows)
    for k in BATCH_ARRAYS:
        a = getattr(batch, k)[other]
        assert (a.tobytes() == getattr(base, k)[other].tobytes()) if base is not None else not a.any(), k
    _check_cert(cert, eff, n_new, nf - n_in)


@pytest.mark.parametrize("name", ["empty", "grazing"])
def test_gpu_depth_surfels_empty(ctx, name):
    ref = DC.reference(name)
    DC.check_conditions(ref)
    assert ref["n_new"] == 0
    batch, cert, eff = _run(ctx, name)
    assert batch.n_camera_valid == 0 and batch.n_valid == 0
    for k in BATCH_ARRAYS:
        a = getattr(batch, k)
        assert np.all(np.isfinite(a.astype(np.float64))) and not a.any(), k
    assert (batch.depth_slot_cells == -1).all() and batch.depth_slot_cells.shape == (ref["n_feat"],)
    _check_cert(cert, eff, 0, ref["n_feat"])
    assert cert.support.ess_total == 0.0
    # no free row: nothing but the record is written either
    full = _base("overflow")
    full.n_camera_valid = full.n_feat
    got, cert, eff = _run(ctx, "overflow", base=full)
    assert got.n_camera_valid == full.n_feat and (got.depth_slot_cells == -1).all()
    for k in BATCH_ARRAYS:
        assert getattr(got, k).tobytes() == getattr(full, k).tobytes(), k
    _check_cert(cert, eff, 0, 0)


def test_gpu_depth_surfels_base_batch(ctx):
    """Rows this call did not write come back bitwise, camera rows below n_camera_valid and the whole LiDAR
    slice included, for a host base and a device-resident base; the new rows are bitwise the no-base run's
    (`overflow` with the same 13 free rows: a base-less run whose budget is 13)."""
    c = DC.build("overflow")
    cfg = DepthSurfelConfig(**c["cfg"])
    nf, n_in = cfg.n_feat, c["base"]
    plain, _, _ = extract_depth_surfels(c["depth"], c["rgb"], PinholeIntrinsics(*c["K"]), c["R"], c["t"], c["timestamp"],
                                        DepthSurfelConfig(**dict(c["cfg"], n_feat=nf - n_in)), ctx=ctx)
    assert plain.n_camera_valid == nf - n_in == 13
    want = _base("overflow")
    for base in (_base("overflow"), _base("overflow", ctx)):
        got, cert, eff = _run(ctx, "overflow", base=base)
        assert (got.n_camera_valid, got.n_lidar_valid, got.n_valid) == (nf, want.n_lidar_valid, nf + want.n_lidar_valid)
        for k in BATCH_ARRAYS:
            g, p, w = getattr(got, k), getattr(plain, k), getattr(want, k)
            assert g[:n_in].tobytes() == w[:n_in].tobytes(), k
            assert g[nf:].tobytes() == w[nf:].tobytes() and w[nf:].any(), k
            if k != "source_indices":  # source_indices = the row, which the base moves by n_in
                assert g[n_in:nf].tobytes() == p[:nf - n_in].tobytes(), k
        np.testing.assert_array_equal(got.source_indices[n_in:nf], np.arange(n_in, nf))
        np.testing.assert_array_equal(got.depth_slot_cells[n_in:], plain.depth_slot_cells)
        assert (got.depth_slot_cells[:n_in] == -1).all()
        _check_cert(cert, eff, 13, 13)
    # fewer valid cells than free rows: the unused camera rows keep the base's values too
    c = DC.build("planes")
    cfg = DepthSurfelConfig(**c["cfg"])
    b = DC.base_arrays(cfg.n_feat, cfg.n_surfel, 2)
    base = MeasurementBatch(**{k: np.array(b[k]) for k in BATCH_ARRAYS}, n_feat=cfg.n_feat, n_surfel=cfg.n_surfel,
                            n_camera_valid=2, n_lidar_valid=2)
    got, _, _ = _run(ctx, "planes", base=base)
    plain, _, _ = _run(ctx, "planes")
    n_new = plain.n_camera_valid
    assert got.n_camera_valid == 2 + n_new < cfg.n_feat
    for k in BATCH_ARRAYS:
        g = getattr(got, k)
        assert g[:2].tobytes() == getattr(base, k)[:2].tobytes() and g[2 + n_new:].tobytes() == getattr(base, k)[2 + n_new:].tobytes(), k
        if k != "source_indices":
            assert g[2:2 + n_new].tobytes() == getattr(plain, k)[:n_new].tobytes(), k


def test_gpu_depth_surfels_reproducible(ctx):
    c = DC.build("overflow")
    a, _, _ = _run(ctx, "overflow")
    b, _, _ = _run(ctx, "overflow")
    _same(a, b)
    dd = _abi.DeviceArray.from_host(ctx, c["depth"], np.float32)
    dc = _abi.DeviceArray.from_host(ctx, c["rgb"], np.uint8)
    args = (PinholeIntrinsics(*c["K"]), c["R"], c["t"], c["timestamp"], DepthSurfelConfig(**c["cfg"]))
    d, _, _ = extract_depth_surfels(dd, dc, *args, base_batch=_base("overflow"), ctx=ctx)
    _same(a, d)
    e, _, _ = extract_depth_surfels(dd, dc, *args, base_batch=_base("overflow"), ctx=ctx, device_out=True)
    assert e.device is not None and all(isinstance(getattr(e, k), _abi.DeviceArray) for k in BATCH_ARRAYS)
    assert all(e.device[k] is getattr(e, k) for k in BATCH_ARRAYS) and isinstance(e.depth_slot_cells, _abi.DeviceArray)
    host = MeasurementBatch(**{k: e.device[k].download().astype(BATCH_ARRAYS[k][1]) for k in BATCH_ARRAYS},
                            n_feat=e.n_feat, n_surfel=e.n_surfel, n_camera_valid=e.n_camera_valid,
                            n_lidar_valid=e.n_lidar_valid, depth_slot_cells=e.depth_slot_cells.download())
    _same(a, host)


COLOUR = (200, 17, 101)


def _uniform_frame(depth_m):
    """A tilted plane about depth_m ahead of a camera at the body, one colour: (depth, rgb, intrinsics)."""
    K, H, W = (57.6, 57.6, 32.0, 24.0), 48, 64
    nrm = np.array([0.2, -0.3, 1.0]) / np.linalg.norm([0.2, -0.3, 1.0])
    i, j = np.mgrid[0:H, 0:W]
    d = np.stack([(j + 0.5 - K[2]) / K[0], (i + 0.5 - K[3]) / K[1], np.ones((H, W))], axis=-1)
    rgb = np.empty((H, W, 3), np.uint8)
    rgb[...] = COLOUR
    return (depth_m / (d @ nrm)).astype(np.float32), rgb, PinholeIntrinsics(*K)


def test_gpu_depth_surfels_map_chain(ctx):
    """extract_depth_surfels(device_out=True) of a uniform-colour frame through MapBranch.front / update on an
    empty map: the inserted slots have source 0 and that colour; the same chain fed the downloaded batch gives
    the same bytes."""
    from gcslam.map_branch import MapBranch
    from gcslam.primitive_map import DevicePrimitiveMap
    from test_gpu_mapbranch import _bits, _branch_config
    depth, rgb, K = _uniform_frame(1.0)
    batch, _, _ = extract_depth_surfels(depth, rgb, K, timestamp_sec=0.5, config=DepthSurfelConfig(n_feat=16, n_surfel=8),
                                        ctx=ctx, device_out=True)
    assert batch.device is not None and batch.n_camera_valid == 12 and batch.n_lidar_valid == 0
    host = _Obj(**{k: batch.device[k].download() for k in BATCH_ARRAYS})
    host.valid_mask = host.valid_mask.astype(bool)
    cfg = _branch_config(16, 8, 8)
    centre, pose = np.array([0.0, 0.0, 1.0]), np.zeros(6)
    maps = []
    for b in (batch, host):
        dm = DevicePrimitiveMap(9, 64, ctx=ctx)
        br = MapBranch(dm, cfg)
        front = br.front(b, centre, pose[None], 1)
        res, _, _ = br.update(front, pose, 0.5)
        assert res.n_inserted > 0
        maps.append((dm, res))
    (dm, res), (dm2, res2) = maps
    assert res.n_inserted == res2.n_inserted and _bits(dm.download()) == _bits(dm2.download())
    got = dm.download("valid_mask", "cam_mass", "lidar_mass", "colors")
    live = got["valid_mask"].astype(bool).reshape(-1)
    assert 0 < live.sum() <= res.n_inserted  # the maintenance behind the insert may merge, it adds none
    # source 0: all of a slot's mass is camera mass (the insert's provenance rule)
    assert (got["cam_mass"].reshape(-1)[live] > 0.0).all() and not got["lidar_mass"].reshape(-1)[live].any()
    np.testing.assert_allclose(got["colors"].reshape(-1, 3)[live], np.broadcast_to(np.array(COLOUR) / 255.0, (live.sum(), 3)),
                               rtol=0.0, atol=1e-12)


def test_gpu_depth_surfels_scan_step(ctx):
    """PrimitiveScanStep.run at H = 2 with depth_frame = {..., "surfels": True}: the camera slice of the scan's
    batch is filled before the front, the new certificate follows the surfel one and is in the GC_LIDAR_CERT
    aggregate, and camera rows reach the map; without the key the camera slice stays empty; with points that
    give no LiDAR surfel the step runs on the frame's rows alone."""
    from gcslam.map_branch import MapBranch
    from gcslam.ops.lidar_surfel_extraction import SurfelExtractionConfig
    from gcslam.primitive_step import PrimitiveScanStep, lidar_cert_row
    from test_gpu_mapbranch import _branch_config
    from test_gpu_mapupdate import _fresh_map
    from test_gpu_primstep import _pipe, _step_case
    import mapupdate_cases as MC
    scfg = SurfelExtractionConfig(n_surfel=64, n_feat=16, voxel_size_m=1.0, min_points_per_voxel=5, hex3d_num_cells_1=8,
                                  hex3d_num_cells_2=8, hex3d_num_cells_z=4, hex3d_max_occupants=32)
    mcase = MC.build("ragged")
    cfg = _branch_config(mcase["m_view"], mcase["K"], mcase["k_ins"])
    case = _step_case(1)
    s = case["scans"][0]
    depth, rgb, K = _uniform_frame(0.6)
    frame = dict(depth=depth, rgb=rgb, intrinsics=K)
    out = {}
    from dataclasses import replace
    for key in (True, None, "rgbd_only"):
        dm = _fresh_map(ctx, mcase)
        before = dm.download("valid_mask", "cam_mass", "lidar_mass")
        step = PrimitiveScanStep(_pipe(case, ctx, False), MapBranch(dm, cfg),
                                 replace(scfg, min_points_per_voxel=1 << 20) if key == "rgbd_only" else scfg)
        r = step.run(0, s, MC.SCAN_SEQ, MC.TIMESTAMP, depth_frame=dict(frame, surfels=True) if key else frame)
        out[key] = (r, dm, before)
    r, dm, before = out[True]
    mb = r.front.measurement_batch
    assert mb.n_camera_valid == 12 and mb.n_lidar_valid >= 8 and mb.device is not None
    np.testing.assert_array_equal(mb.depth_slot_cells.download()[:12], np.arange(12))
    names = [c.anchor_id for c in r.certs]
    assert names[:4] == ["deskew_constant_twist", "surfel_extraction", "depth_surfel_extraction",
                         "primitive_map_recency_inflate"], names
    assert r.certs[2].approximation_triggers == TRIGGERS and r.certs[2].support.ess_total == 12.0
    assert r.certs[2].support.support_frac == 12.0 / 16.0
    row = lidar_cert_row(r.certs[:3] + r.certs[4:], [r.certs[3]])
    assert r.lidar_cert.tobytes() == row.tobytes()
    # camera rows were inserted: the plan names rows below n_feat, and the map holds more source-0 primitives (camera mass only)
    plan = r.update[0]
    cam_inserted = plan.insert_valid.astype(bool) & (plan.insert_indices < mb.n_feat)
    assert cam_inserted.any()
    after = dm.download("valid_mask", "cam_mass", "lidar_mass")
    count = lambda m: int((m["valid_mask"].astype(bool).reshape(-1) & (m["cam_mass"].reshape(-1) > 0.0) &
                           (m["lidar_mass"].reshape(-1) == 0.0)).sum())  # slots whose mass is all camera mass: source 0
    assert count(after) > count(before)
    # a scan whose points give no LiDAR surfel still runs: the frame's rows are the whole batch
    r1, _, _ = out["rgbd_only"]
    mb1 = r1.front.measurement_batch
    assert mb1.n_lidar_valid == 0 and mb1.n_camera_valid == 12 and r1.certs[1].support.ess_total == 0.0
    assert np.all(np.isfinite(r1.z_t)) and np.all(np.isfinite(r1.lidar_cert))
    assert (r1.update[0].insert_valid.astype(bool) & (r1.update[0].insert_indices < mb1.n_feat)).any()
    # without the key: the step as it was
    r0, _, _ = out[None]
    assert r0.front.measurement_batch.n_camera_valid == 0 and r0.front.measurement_batch.depth_slot_cells is None
    assert [c.anchor_id for c in r0.certs] == names[:2] + names[3:]
    assert r0.front.measurement_batch.n_lidar_valid == mb.n_lidar_valid
