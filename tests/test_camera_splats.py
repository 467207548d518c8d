"""Camera splats without a GPU: the fixture recorded from the reference's own NumPy code
(tests/golden/camera_splats.npz, tests/golden/make_camera_splats.py), the conditions under which its
cases pin a device implementation, the restatement (tests/camsplat_restatement.py) held to the
recorded outputs, and the Python layer's argument checks, empty batch and feature packing.

Restatement against the reference, worst |difference| / max |reference| over the five cases (printed
by test_restatement_matches_reference): see DESIGN.md §4; the bar is 1e-12, the bar at which the
oracle is held to the reference's CSV outputs."""

import types

import numpy as np
import pytest

import camsplat_cases as CC
import camsplat_restatement as RS
from gcslam import _abi
from gcslam.measurement_batch import BATCH_ARRAYS
from gcslam.ops import (CameraFeatures, LidarCameraDepthFusionConfig, MeasurementBatch, PinholeIntrinsics,
                        camera_measurement_batch, feature_list_to_camera_batch, lidar_depth_evidence,
                        measurement_batch_from_camera_splats)
from gcslam.ops import camera_splats as CS

NAMES = list(CC.CASES)
BAR = 1e-12
K = (CC.FX, CC.FY, CC.CX, CC.CY)


@pytest.fixture(scope="module")
def cases():
    g = np.load(CC.GOLDEN)
    return {n: CC.load(n, g) for n in NAMES}


@pytest.fixture(scope="module")
def restated(cases):
    return {(n, w): CC.restated(cases[n], weighted=w) for n in NAMES for w in (True, False)}


@pytest.mark.parametrize("name", NAMES)
def test_fixture_holds_the_cases(cases, name):
    built, c = CC.build(name), cases[name]
    for k in CC.INPUT_KEYS:
        if built[k] is None:
            assert c.get(k) is None
        else:
            assert np.asarray(c[k]).tobytes() == built[k].tobytes(), k
    for k, v in built["features"].items():
        assert np.asarray(c["features"][k]).tobytes() == np.asarray(v).tobytes(), k
    assert np.array_equal(c["points_cam"], RS.to_camera_frame(c["points_base"], CC.R_BASE_CAMERA, CC.T_BASE_CAMERA))


@pytest.mark.parametrize("name", NAMES)
def test_conditions(cases, restated, name):
    """The cases stay away from every place where a last-bit difference changes the answer."""
    c = cases[name]
    cfg = CC.config(c)
    for weighted in (True, False):
        cd = restated[name, weighted]["cond"]
        sup = cd["supported"]
        assert cd["radius_margin"] >= 1e-9, cd["radius_margin"]
        assert np.min(cd["kth_gap"]) >= 1e-9
        assert np.min(np.abs(cd["n_z"][sup])) >= 1e-6
        zr = cd["z_raw"][sup] - cfg.depth_min_m
        assert np.min(np.abs(zr)) >= 1e-6 and np.min(np.abs(np.abs(zr) - 20.0)) >= 1e-6
        undet = int((~RS.determined(cd)).sum())
        assert undet <= 0.10 * sup.sum(), (undet, int(sup.sum()))


def test_coverage(cases, restated):
    mixed, cfg = restated["mixed", False]["cond"], CC.config(cases["mixed"])
    cnt, sup = mixed["counts"], mixed["supported"]
    assert (cnt < cfg.lidar_plane_fit_min_points).sum() >= 2
    assert (cnt == cfg.lidar_plane_fit_min_points).sum() >= 1
    assert (sup & (cnt % 2 == 0)).sum() >= 5 and (sup & (cnt % 2 == 1)).sum() >= 5
    zr = mixed["z_raw"][sup] - cfg.depth_min_m
    assert (zr < 0.0).sum() >= 1 and (zr > 20.0).sum() >= 1  # both softplus / behind branches
    sel = restated["select", True]["cond"]
    assert (sel["counts"] > CC.config(cases["select"]).lidar_ray_plane_fit_max_points).sum() >= 20
    t = cases["truncate"]
    fused, Lc = t["ref_fused_flag"], t["features"]["depth_Lambda_c"]
    assert (~fused).sum() >= 1
    assert (fused & (Lc == 0.0)).sum() >= 10
    assert (fused & (Lc > 0.0) & (t["ref_Lambda_ell"] > 0.0)).sum() >= 10
    assert t["uv"].shape[0] > t["n_feat"] and cases["pad"]["uv"].shape[0] < cases["pad"]["n_feat"]


def test_restatement_matches_reference(cases, restated):
    worst = {}
    for name in NAMES:
        c = cases[name]
        for weighted, tag in ((True, "ref_"), (False, "ref_plain_")):
            if tag + "Lambda_ell" not in c:
                continue
            ev = restated[name, weighted]
            cd = ev["cond"]
            np.testing.assert_array_equal(cd["counts"] >= CC.config(c).lidar_plane_fit_min_points, cd["supported"])
            det = RS.determined(cd)
            for k in RS.EV_KEYS:
                rows = None if k in ("Lambda_A", "theta_A") else det
                worst[k] = max(worst.get(k, 0.0), CC.err_frac(ev[k], c[tag + k], BAR, rows))
        ev = restated[name, False]
        xyz, cov, flag = RS.fuse(c["features"], ev["Lambda_ell"], ev["theta_ell"], *K, CC.config(c))
        np.testing.assert_array_equal(flag, c["ref_fused_flag"])
        det = RS.determined(ev["cond"])
        worst["fused_xyz"] = max(worst.get("fused_xyz", 0.0), CC.err_frac(xyz, c["ref_fused_xyz"], BAR, det))
        worst["fused_cov"] = max(worst.get("fused_cov", 0.0), CC.err_frac(cov, c["ref_fused_cov"], BAR, det))
    print("restatement vs reference, fraction of the 1e-12 bar:", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_abi, "lib", boom)
    monkeypatch.setattr(_abi, "default_context", boom)
    monkeypatch.setattr(_abi, "call", boom)


def _feats(m=2, **over):
    f = CC.features(np.full((m, 2), 10.0))
    f.update(over)
    return CameraFeatures(**f)


def test_argument_errors_need_no_library(monkeypatch):
    _no_device(monkeypatch)
    pts, uv, C = np.ones((4, 3)), np.ones((2, 2)), LidarCameraDepthFusionConfig
    bad_cfg = [C(lidar_ray_plane_fit_max_points=257), C(lidar_ray_plane_fit_max_points=0),
               C(lidar_plane_fit_min_points=0), C(lidar_projection_radius_pix=0.0),
               C(lidar_projection_radius_pix=float("inf")), C(gamma_lidar=float("nan"))]
    for cfg in bad_cfg:
        with pytest.raises(ValueError):
            lidar_depth_evidence(pts, uv, *K, cfg)
    for k in ((0.0, 75.0, 1.0, 1.0), (75.0, 0.0, 1.0, 1.0), (75.0, 75.0, float("nan"), 1.0), (float("inf"), 1.0, 1.0, 1.0)):
        with pytest.raises(ValueError):
            lidar_depth_evidence(pts, uv, *k, C())
    big = np.broadcast_to(np.zeros(3), ((1 << 22) + 1, 3))
    for kw in (dict(points_camera_frame=big, uv_query=uv), dict(points_camera_frame=pts, uv_query=np.zeros((4097, 2))),
               dict(points_camera_frame=np.ones((4, 2)), uv_query=uv), dict(points_camera_frame=pts, uv_query=np.ones((2, 3))),
               dict(points_camera_frame=pts, uv_query=uv, point_weights=np.ones(3))):
        with pytest.raises(ValueError):
            lidar_depth_evidence(fx=75.0, fy=75.0, cx=1.0, cy=1.0, config=C(), **kw)
    intr, R, t = PinholeIntrinsics(*K), np.eye(3), np.zeros(3)
    run = lambda **kw: camera_measurement_batch(**{**dict(points_base=pts, features=_feats(), intrinsics=intr,
                                                           R_base_camera=R, t_base_camera=t, timestamp_sec=1.0,
                                                           config=C(), n_feat=4, n_surfel=2), **kw})
    for kw in (dict(config=bad_cfg[0]), dict(intrinsics=PinholeIntrinsics(0.0, 1.0, 1.0, 1.0)), dict(points_base=big),
               dict(n_feat=-1), dict(n_surfel=1.5), dict(R_base_camera=np.eye(2)), dict(t_base_camera=np.full(3, np.nan)),
               dict(pixel_sigma=float("nan")), dict(features=_feats(xyz=np.ones((3, 3)))),
               dict(features=_feats(has_color=np.ones(3, bool))), dict(features=_feats(4097))):
        with pytest.raises(ValueError):
            run(**kw)
    ok = dict(positions=np.ones((2, 3)), covariances=np.tile(np.eye(3), (2, 1, 1)), directions=np.ones((2, 3)),
              kappas=np.ones(2), weights=np.ones(2), timestamps=np.ones(2))
    for kw in (dict(covariances=np.ones((3, 3, 3))), dict(kappas=np.ones(3)), dict(colors=np.ones((1, 3))),
               dict(n_feat=-2), dict(eps_lift=float("nan")), dict(positions=np.ones((2, 2)))):
        with pytest.raises(ValueError):
            measurement_batch_from_camera_splats(**{**ok, **kw})
    with pytest.raises(ValueError):
        feature_list_to_camera_batch([object()], 0.0, n_feat=-1)


def _is_empty(b, n_feat, n_surfel):
    assert isinstance(b, MeasurementBatch) and b.device is None
    assert (b.n_feat, b.n_surfel, b.n_camera_valid, b.n_lidar_valid) == (n_feat, n_surfel, 0, 0)
    for k, (shp, dt, _) in BATCH_ARRAYS.items():
        a = getattr(b, k)
        assert a.shape == (n_feat + n_surfel,) + shp and a.dtype == dt and not a.any(), k


def test_no_features_give_the_empty_batch(monkeypatch):
    _no_device(monkeypatch)
    b = camera_measurement_batch(np.ones((5, 3)), _feats(0), PinholeIntrinsics(*K), np.eye(3), np.zeros(3), 2.0,
                                 n_feat=6, n_surfel=3)
    _is_empty(b, 6, 3)
    b, diag = camera_measurement_batch(np.zeros((0, 3)), _feats(0), PinholeIntrinsics(*K), np.eye(3), np.zeros(3), 2.0,
                                       n_feat=2, n_surfel=0, return_diag=True)
    _is_empty(b, 2, 0)
    assert diag is None
    _is_empty(feature_list_to_camera_batch([], 1.0, n_feat=3, n_surfel=4), 3, 4)
    L, th, diag = lidar_depth_evidence(np.ones((5, 3)), np.zeros((0, 2)), *K, return_diag=True)
    assert L.shape == th.shape == (0,)
    assert set(diag) == {"Lambda_A", "theta_A", "Lambda_B", "theta_B", "z_B", "sigma_sq_B", "w_B", "n_in_radius"}
    assert all(v.shape == (0,) for v in diag.values())


def test_feature_list_packing(monkeypatch):
    """Duck-typed features -> the arrays the tail entry takes (camera_batch_utils.py:39-65)."""
    seen = {}

    def capture(positions, covariances, directions, kappas, weights, timestamps, colors, **kw):
        seen.update(positions=positions, covariances=covariances, directions=directions, kappas=kappas,
                    weights=weights, timestamps=timestamps, colors=colors, **kw)
        return "batch"
    monkeypatch.setattr(CS, "measurement_batch_from_camera_splats", capture)
    rng = np.random.default_rng(5)
    fs = []
    for i in range(5):
        f = types.SimpleNamespace(xyz=rng.uniform(1, 2, 3), cov_xyz=np.eye(3) * (i + 1.0), weight=0.1 * (i + 1),
                                  kappa_app=2.0 + i, mu_app=rng.standard_normal(3) if i % 2 == 0 else None)
        if i != 1:  # a feature type without the attribute at all
            f.color = [0.2 * i, 1.5, -0.5] if i != 3 else None
        fs.append(f)
    assert feature_list_to_camera_batch(fs, 7.5, n_feat=4, n_surfel=2, eps_lift=1e-6) == "batch"
    n = 4  # truncated to n_feat
    assert seen["n_feat"] == 4 and seen["n_surfel"] == 2 and seen["eps_lift"] == 1e-6
    np.testing.assert_array_equal(seen["positions"], np.array([f.xyz for f in fs[:n]]))
    np.testing.assert_array_equal(seen["covariances"], np.array([f.cov_xyz for f in fs[:n]]))
    np.testing.assert_array_equal(seen["weights"], [f.weight for f in fs[:n]])
    np.testing.assert_array_equal(seen["kappas"], [f.kappa_app for f in fs[:n]])
    np.testing.assert_array_equal(seen["timestamps"], np.full(n, 7.5))
    np.testing.assert_array_equal(seen["colors"], [[0.0, 1.5, -0.5], [0.5] * 3, [0.4, 1.5, -0.5], [0.5] * 3])
    for i, f in enumerate(fs[:n]):
        d = np.asarray(f.mu_app if f.mu_app is not None else f.xyz, np.float64)
        np.testing.assert_array_equal(seen["directions"][i], d / (np.linalg.norm(d) + 1e-12))


def test_config_has_the_reference_fields():
    c = LidarCameraDepthFusionConfig()
    assert len(CS._cfg(c)._fields_) == 23
    assert (c.lidar_projection_radius_pix, c.lidar_plane_fit_min_points, c.lidar_ray_plane_fit_max_points) == (3.0, 3, 64)
    assert (c.depth_min_m, c.depth_sigma_max_sq, c.depth_min_sigmoid_alpha_z, c.gamma_lidar) == (0.05, 1e4, 20.0, 1.0)
    with pytest.raises(Exception):
        c.gamma_lidar = 2.0  # frozen, as in the reference
