"""Camera splats on the device (gc_camsplat.hip, gcslam/ops/camera_splats.py) against the outputs the
reference's own NumPy code gave for the same inputs (tests/golden/camera_splats.npz), and against the
restatement (tests/camsplat_restatement.py) for the two steps the reference has only as node / JAX
code: the base-frame loop and measurement_batch_from_camera_splats. The conditions under which the
cases pin an implementation are asserted in test_camera_splats.py.

Counts, flags, masks, sources and indices are compared exactly; every float array at 1e-10 of the
reference array's max-abs (the bar of the surfel and VisualPoseEvidence operators). A plane normal is
an eigenvector: Route B's outputs and what is fused from them are compared where
(λ1 − λ0) / λ2 >= 1e-4 (camsplat_restatement.determined). The measured fractions of the bar are
printed by test_gpu_camsplat_parity and recorded in DESIGN.md §4."""

import numpy as np
import pytest

import camsplat_cases as CC
import camsplat_restatement as RS
from gcslam import _abi
from gcslam.measurement_batch import BATCH_ARRAYS
from gcslam.ops import (CameraFeatures, MeasurementBatch, PinholeIntrinsics, SurfelExtractionConfig,
                        camera_measurement_batch, extract_lidar_surfels, lidar_depth_evidence,
                        measurement_batch_from_camera_splats)

BAR = 1e-10
K = (CC.FX, CC.FY, CC.CX, CC.CY)
INTR = PinholeIntrinsics(*K)
FLOATS = ("Lambdas", "thetas", "etas", "weights", "timestamps", "colors")
EXACT = ("sources", "source_indices", "valid_mask")


@pytest.fixture(scope="module")
def cases():
    g = np.load(CC.GOLDEN)
    return {n: CC.load(n, g) for n in CC.CASES}


def _fused(ctx, c, points=None, **kw):
    return camera_measurement_batch(c["points_base"] if points is None else points, CameraFeatures(**c["features"]), INTR,
                                    CC.R_BASE_CAMERA, CC.T_BASE_CAMERA, CC.TIMESTAMP, CC.config(c), n_feat=c["n_feat"],
                                    n_surfel=c["n_surfel"], eps_lift=CC.EPS_LIFT, ctx=ctx, **kw)


def _bytes_equal(a: MeasurementBatch, b: MeasurementBatch):
    for k in BATCH_ARRAYS:
        x, y = np.asarray(getattr(a, k)), np.asarray(getattr(b, k))
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert (a.n_feat, a.n_surfel, a.n_camera_valid, a.n_lidar_valid) == (b.n_feat, b.n_surfel, b.n_camera_valid,
                                                                         b.n_lidar_valid)


def _check_batch(batch, want, rows_ok, worst):
    """batch against the dict of camsplat_restatement.batch_rows; float rows compared where rows_ok."""
    nv, nt = want["n_camera_valid"], want["Lambdas"].shape[0]
    assert isinstance(batch, MeasurementBatch) and batch.n_camera_valid == nv and batch.n_lidar_valid == 0
    for k, (shp, dt, _) in BATCH_ARRAYS.items():
        a = getattr(batch, k)
        assert a.shape == (nt,) + shp and a.dtype == dt, k
        assert not a[nv:].any(), k  # a complete fresh batch: every other row zero
    for k in EXACT:
        np.testing.assert_array_equal(getattr(batch, k), want[k], err_msg=k)
    ok = np.zeros(nt, bool)
    ok[:nv] = rows_ok[:nv]
    for k in FLOATS:
        worst[k] = max(worst.get(k, 0.0), CC.err_frac(getattr(batch, k), want[k], BAR, ok))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CC.CASES))
def test_gpu_camsplat_parity(ctx, cases, name):
    c = cases[name]
    batch, diag = _fused(ctx, c, return_diag=True)
    tag = "ref_plain_" if "ref_plain_Lambda_ell" in c else "ref_"  # the fused call passes no point weights
    cond = CC.restated(c, weighted=False)["cond"]
    det = RS.determined(cond)
    np.testing.assert_array_equal(diag.n_in_radius, cond["counts"])
    np.testing.assert_array_equal(diag.fused, c["ref_fused_flag"])
    worst = {}
    for k in RS.EV_KEYS:
        rows = None if k in ("Lambda_A", "theta_A") else det
        worst[k] = CC.err_frac(getattr(diag, k), c[tag + k], BAR, rows)
    worst["fused_xyz"] = CC.err_frac(diag.xyz, c["ref_fused_xyz"], BAR, det)
    worst["fused_cov"] = CC.err_frac(diag.cov_xyz, c["ref_fused_cov"], BAR, det)
    _check_batch(batch, CC.expected_batch(c), det, worst)
    assert batch.n_camera_valid == min(c["uv"].shape[0], c["n_feat"]) and batch.device is None
    assert not batch.etas[:, 1:].any()
    print(name, "fraction of the 1e-10 bar:", {k: float("%.3g" % v) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.gpu
def test_gpu_lidar_depth_evidence_alone(ctx, cases):
    for name, weighted in (("select", True), ("select", False), ("mixed", False), ("smallest", False)):
        c = cases[name]
        tag = "ref_" if weighted or "ref_plain_Lambda_ell" not in c else "ref_plain_"
        pw = c["point_weights"] if weighted else None
        cond = CC.restated(c, weighted=weighted)["cond"]
        det = RS.determined(cond)
        L, th, diag = lidar_depth_evidence(c["points_cam"], c["uv"], *K, CC.config(c), point_weights=pw,
                                           return_diag=True, ctx=ctx)
        assert set(diag) == {"Lambda_A", "theta_A", "Lambda_B", "theta_B", "z_B", "sigma_sq_B", "w_B", "n_in_radius"}
        np.testing.assert_array_equal(diag["n_in_radius"], cond["counts"])
        got = dict(diag, Lambda_ell=L, theta_ell=th)
        for k in RS.EV_KEYS:
            rows = None if k in ("Lambda_A", "theta_A") else det
            assert CC.err_frac(got[k], c[tag + k], BAR, rows) <= 1.0, (name, weighted, k)
        L2, th2 = lidar_depth_evidence(c["points_cam"], c["uv"], *K, CC.config(c), point_weights=pw, ctx=ctx)
        assert L2.tobytes() == L.tobytes() and th2.tobytes() == th.tobytes() and L.shape == (c["uv"].shape[0],)
    c = cases["select"]  # the weights change the plane fit
    a = lidar_depth_evidence(c["points_cam"], c["uv"], *K, CC.config(c), point_weights=c["point_weights"], ctx=ctx)
    b = lidar_depth_evidence(c["points_cam"], c["uv"], *K, CC.config(c), ctx=ctx)
    assert a[0].tobytes() != b[0].tobytes()
    one = lidar_depth_evidence(c["points_cam"], c["uv"][3], *K, CC.config(c), ctx=ctx)  # a single (u, v)
    assert one[0].shape == (1,) and one[0][0] == b[0][3]


@pytest.mark.gpu
def test_gpu_batch_from_camera_splats_alone(ctx):
    rng = np.random.default_rng(3)
    for n, n_feat, n_surfel, with_colors in ((7, 5, 3, True), (3, 5, 2, False), (5, 5, 0, True)):
        A = rng.standard_normal((n, 3, 3)) * 0.1
        args = dict(positions=rng.uniform(-3, 3, (n, 3)), covariances=A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3),
                    directions=rng.standard_normal((n, 3)), kappas=rng.uniform(0.1, 9.0, n),
                    weights=rng.uniform(0.1, 1.0, n), timestamps=rng.uniform(5.0, 6.0, n),
                    colors=rng.uniform(-0.1, 1.1, (n, 3)) if with_colors else None)
        want = RS.batch_rows(**args, n_feat=n_feat, n_surfel=n_surfel, eps_lift=1e-7)
        got = measurement_batch_from_camera_splats(**args, n_feat=n_feat, n_surfel=n_surfel, eps_lift=1e-7, ctx=ctx)
        worst = {}
        _check_batch(got, want, np.ones(n_feat + n_surfel, bool), worst)
        assert max(worst.values()) <= 1.0, worst
        assert (got.n_feat, got.n_surfel) == (n_feat, n_surfel)
        if not with_colors:
            assert (got.colors[:n] == 0.5).all()
        dev = measurement_batch_from_camera_splats(**{k: (_abi.DeviceArray.from_host(ctx, v) if v is not None else None)
                                                      for k, v in args.items()}, n_feat=n_feat, n_surfel=n_surfel,
                                                   eps_lift=1e-7, ctx=ctx, device_out=True)
        assert dev.device is not None and all(dev.device[k] is getattr(dev, k) for k in BATCH_ARRAYS)
        host = MeasurementBatch(**{k: dev.device[k].download().astype(BATCH_ARRAYS[k][1]) for k in BATCH_ARRAYS},
                                n_feat=n_feat, n_surfel=n_surfel, n_camera_valid=dev.n_camera_valid, n_lidar_valid=0)
        _bytes_equal(got, host)


@pytest.mark.gpu
def test_gpu_camsplat_reproducible(ctx, cases):
    c = cases["truncate"]
    a, da = _fused(ctx, c, return_diag=True)
    b, db = _fused(ctx, c, return_diag=True)
    _bytes_equal(a, b)
    for k in da.__dataclass_fields__:
        assert getattr(da, k).tobytes() == getattr(db, k).tobytes(), k
    dp = _abi.DeviceArray.from_host(ctx, c["points_base"])
    d, dd = _fused(ctx, c, points=dp, return_diag=True)
    _bytes_equal(a, d)
    assert dd.xyz.tobytes() == da.xyz.tobytes() and dd.Lambda_ell.tobytes() == da.Lambda_ell.tobytes()
    e = _fused(ctx, c, points=dp, device_out=True)
    assert e.device is not None and all(isinstance(getattr(e, k), _abi.DeviceArray) for k in BATCH_ARRAYS)
    host = MeasurementBatch(**{k: e.device[k].download().astype(BATCH_ARRAYS[k][1]) for k in BATCH_ARRAYS},
                            n_feat=e.n_feat, n_surfel=e.n_surfel, n_camera_valid=e.n_camera_valid, n_lidar_valid=0)
    _bytes_equal(a, host)


class _Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.gpu
def test_gpu_camsplat_device_chain(ctx, cases):
    """camera_measurement_batch(device_out) -> extract_lidar_surfels(base_batch, device_out) ->
    associate_primitives_ot, all in HBM: the camera slice is what the first call wrote, the LiDAR slice
    what a surfel call on an empty base writes, the association that of the same batch from the host."""
    import surfel_cases as SC
    from gcslam.association import AssociationConfig, associate_primitives_ot, extract_atlas_map_view
    from test_association import _device_map, _hex_map
    c = dict(cases["mixed"], n_feat=64, n_surfel=64)
    s = SC.build("overflow_truncate")
    scfg = SurfelExtractionConfig(**dict(s["cfg"], n_feat=64))
    assert scfg.n_surfel == 64
    cam_host = _fused(ctx, c)
    cam = _fused(ctx, c, device_out=True)
    full, _, _ = extract_lidar_surfels(s["points"], s["timestamps"], s["weights"], scfg, base_batch=cam, ctx=ctx,
                                       device_out=True)
    plain, _, _ = extract_lidar_surfels(s["points"], s["timestamps"], s["weights"], scfg, ctx=ctx)
    nf, nv = 64, plain.n_lidar_valid
    assert (full.n_camera_valid, full.n_lidar_valid) == (cam_host.n_camera_valid, nv) and nv > 0
    host = _Obj(**{k: full.device[k].download() for k in BATCH_ARRAYS})
    for k in BATCH_ARRAYS:
        g = getattr(host, k).astype(BATCH_ARRAYS[k][1])
        assert g[:nf].tobytes() == getattr(cam_host, k)[:nf].tobytes(), k
        assert g[nf:].tobytes() == getattr(plain, k)[nf:].tobytes(), k
    host.valid_mask = host.valid_mask.astype(bool)
    rng = np.random.default_rng(13)
    tiles = _hex_map(rng, 64, 60, [(a, b, cz) for a in range(-1, 1) for b in range(-1, 1) for cz in (-1, 0)])
    view = extract_atlas_map_view(_device_map(ctx, tiles, 64), list(tiles), 32)
    (ra, ca, _), (rb, cb, _) = (associate_primitives_ot(b, view, AssociationConfig(scan_seq=9)) for b in (full, host))
    assert ra.responsibilities.any() and ra.responsibilities[:cam_host.n_camera_valid].any()
    for k in ("responsibilities", "candidate_pool_indices", "candidate_tile_ids", "candidate_slots", "row_masses",
              "cost_matrix"):
        assert getattr(ra, k).tobytes() == getattr(rb, k).tobytes(), k
    assert ca.to_dict() == cb.to_dict()


@pytest.mark.gpu
def test_gpu_camsplat_edges(ctx, cases):
    c = cases["pad"]
    m = c["uv"].shape[0]
    f = c["features"]
    zero = np.zeros(m)
    # no points, and every point behind the camera: no LiDAR evidence, camera-only and fall-back rows
    zc = c["points_cam"][:, 2:3]
    behind = c["points_base"] - (zc + np.abs(zc) + 1.0) * CC.R_BASE_CAMERA[:, 2][None]  # z -> -1 - |z|
    assert (RS.to_camera_frame(behind, CC.R_BASE_CAMERA, CC.T_BASE_CAMERA)[:, 2] < 0.0).all()
    for pts in (np.zeros((0, 3)), behind):
        batch, diag = _fused(ctx, c, points=pts, return_diag=True)
        assert not diag.Lambda_ell.any() and not diag.theta_ell.any() and not diag.n_in_radius.any()
        assert not diag.w_B.any() and np.isnan(diag.z_B).all() and np.isnan(diag.sigma_sq_B).all()
        xyz, cov, flag = RS.fuse(f, zero, zero, *K, CC.config(c))
        np.testing.assert_array_equal(diag.fused, flag)
        assert flag.any() and (~flag).any() and np.array_equal(flag, f["depth_Lambda_c"] > 0.0)
        worst = dict(xyz=CC.err_frac(diag.xyz, xyz, BAR), cov=CC.err_frac(diag.cov_xyz, cov, BAR))
        _check_batch(batch, CC.expected_batch(c, xyz, cov), np.ones(batch.n_total, bool), worst)
        assert max(worst.values()) <= 1.0, worst
        L, th = lidar_depth_evidence(RS.to_camera_frame(pts, CC.R_BASE_CAMERA, CC.T_BASE_CAMERA), c["uv"], *K, ctx=ctx)
        assert L.shape == (m,) and not L.any() and not th.any()
    # more in-radius points than a query can hold: an argument error, and the context stays usable
    rng = np.random.default_rng(2)
    z = rng.uniform(3.0, 3.1, 1100)
    u, v = 40.0 + rng.uniform(-0.4, 0.4, 1100), 30.0 + rng.uniform(-0.4, 0.4, 1100)
    crowd = np.stack([(u - CC.CX) / CC.FX * z, (v - CC.CY) / CC.FY * z, z], axis=1)
    with pytest.raises(ValueError, match="GC_CAM_MAX_NEAR"):
        lidar_depth_evidence(crowd, np.array([[40.0, 30.0], [80.0, 60.0]]), *K, ctx=ctx)
    L, _, d = lidar_depth_evidence(crowd[:1000], np.array([[40.0, 30.0], [80.0, 60.0]]), *K, ctx=ctx, return_diag=True)
    assert d["n_in_radius"].tolist() == [1000, 0] and L[0] > 0.0 and L[1] == 0.0
    with pytest.raises(ValueError, match="GC_CAM_MAX_NEAR"):
        _fused(ctx, dict(c, features=dict(f, u=np.full(m, 40.0), v=np.full(m, 30.0))),
               points=crowd @ CC.R_BASE_CAMERA.T + CC.T_BASE_CAMERA)
    a = _fused(ctx, cases["pad"])
    _bytes_equal(a, _fused(ctx, cases["pad"]))
