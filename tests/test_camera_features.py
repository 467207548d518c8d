"""The camera-feature lift without a GPU: known answers for the restatement
(tests/camfeat_restatement.py), the conditions under which the cases (tests/camfeat_cases.py) pin an
implementation, select_keypoints, and every argument error, raised before a device is asked for.
The device parity is test_gpu_camera_features.py."""

import math

import numpy as np
import pytest

import camfeat_cases as FC
import camfeat_restatement as RS
from gcslam import _abi
from gcslam.ops import (CameraFeatures, PinholeIntrinsics, VisualFeatureConfig, lift_camera_features,
                        select_keypoints)
from gcslam.ops import camera_features as CF


def _quadratic_image(coef, u0, v0, shape=(24, 32)):
    """z = c0 + d du + e dv + a du² + b du dv + c dv² about (u0, v0): dyadic coefficients and offsets,
    so every pixel is exact in float32."""
    a, b, c, d, e, c0 = coef
    x, y = np.meshgrid(np.arange(shape[1], dtype=np.float64), np.arange(shape[0], dtype=np.float64))
    du, dv = x - u0, y - v0
    z = c0 + d * du + e * dv + a * du * du + b * du * dv + c * dv * dv
    z32 = z.astype(np.float32)
    assert np.array_equal(z32.astype(np.float64), z)
    return z32


def test_restatement_quadratic_known_answer():
    coef = (1.0 / 64, -1.0 / 128, 1.0 / 32, 1.0 / 16, -1.0 / 8, 4.0)
    u0, v0 = 10.25, 12.5  # v rounds half away, to 13
    fx, fy, cx, cy = 64.0, 32.0, 16.0, 12.0
    depth = _quadratic_image(coef, u0, v0)
    cfg = VisualFeatureConfig(depth_sample_mode="nearest")
    out = RS.lift(depth, None, [[u0, v0, 50.0]], (fx, fy, cx, cy), cfg)
    c = out["cond"]
    assert (c["x"][0], c["y"][0]) == (10, 13) and c["fit"][0] and c["n_fit"][0] == 25 and c["n_window"][0] == 1
    a, b, cc, d, e, c0 = coef
    # the ridge of 1e-8 bounds the bias: |beta - beta0| <= eps |(AtA + eps I)^-1| |beta0| < 1e-6
    np.testing.assert_allclose(c["beta"][0], [a, b, cc, d, e, c0], rtol=0.0, atol=1e-6)
    z_hat = float(depth[13, 10])
    assert out["z_m"][0] == z_hat and out["xyz"][0, 2] == z_hat
    sx, sy = fx / z_hat, fy / z_hat
    zu, zv = sx * d, sy * e
    h00, h01, h11 = sx * sx * 2 * a, sx * sy * b, sy * sy * 2 * cc
    det = h00 * h11 - h01 * h01
    n = np.array([-zu, -zv, 1.0]) / math.sqrt(zu * zu + zv * zv + 1.0)
    lam = 0.5 * (h00 + h11) - math.sqrt(0.25 * (h00 - h11) ** 2 + h01 * h01)
    scale = max(abs(h00), abs(h11))
    np.testing.assert_allclose(out["mu_app"][0], n, rtol=0.0, atol=1e-6)
    assert abs(out["K"][0] - det / (1.0 + zu * zu + zv * zv) ** 2) <= 1e-6 * max(1.0, abs(det))
    assert abs(c["det_ratio"][0] - abs(det) / (h00 * h00 + 2 * h01 * h01 + h11 * h11)) <= 1e-6
    assert abs(out["lam_min"][0] - lam) <= 1e-6 * scale
    assert out["has_mu_app"][0] and not out["has_color"][0] and not out["color"].any()
    # nearest: no window variance, so var_z_eff = depth_sigma² and Lambda_c = 1 / it (:567-569, :605-609)
    sig = 0.01 + 0.01 * z_hat
    assert out["depth_sigma_c_sq"][0] == sig * sig and out["depth_Lambda_c"][0] == 1.0 / (sig * sig)
    assert out["depth_theta_c"][0] == out["depth_Lambda_c"][0] * z_hat
    np.testing.assert_allclose(out["xyz"][0], [(u0 - cx) * z_hat / fx, (v0 - cy) * z_hat / fy, z_hat], rtol=1e-15)


def test_restatement_constant_image_and_rounding():
    depth = np.full((16, 20), 2.5, np.float32)
    rgb = np.arange(16 * 20 * 3, dtype=np.int64).reshape(16, 20, 3).astype(np.uint8)
    kp = [[7.3, 8.1, 10.0],      # interior
          [6.5, 3.0, 10.0],      # u = k + 0.5 rounds up to 7 (np.round would give 6)
          [5.5, 3.0, 10.0],      # to 6 (np.round agrees)
          [-0.4, 4.0, 10.0],     # rounds to -0: inside
          [-0.5, 4.0, 10.0],     # rounds to -1: outside
          [3.0, 15.5, 10.0],     # v rounds to 16 = H: outside
          [3.0, 15.4, 10.0]]
    out = RS.lift(depth, rgb, kp, (20.0, 20.0, 10.0, 8.0), VisualFeatureConfig())
    c = out["cond"]
    assert c["x"].tolist() == [7, 7, 6, 0, -1, 3, 3] and c["y"].tolist() == [8, 3, 3, 4, 4, 16, 15]
    assert c["in_image"].tolist() == [True, True, True, True, False, False, True]
    assert np.array_equal(c["z_valid"], c["in_image"]) and np.array_equal(c["fit"], c["in_image"])
    ok = c["in_image"]
    # (the ridge couples the constant 2.5 into the slopes of a clipped window: a bias below 1e-6)
    np.testing.assert_allclose(out["mu_app"][ok], np.tile([0.0, 0.0, 1.0], (int(ok.sum()), 1)), rtol=0.0, atol=1e-6)
    assert (out["z_m"][ok] == 2.5).all() and np.isnan(out["z_m"][~ok]).all()
    assert c["n_window"].tolist() == [9, 9, 9, 6, 0, 0, 6] and c["n_fit"].tolist() == [25, 25, 25, 15, 0, 0, 15]
    # an invalid row (:574-575, :602-604)
    for i in np.nonzero(~ok)[0]:
        assert not out["xyz"][i].any() and np.array_equal(out["cov_xyz"][i], np.eye(3) * 1e6)
        assert out["weight"][i] == 0.0 and out["depth_Lambda_c"][i] == 0.0 and out["depth_theta_c"][i] == 0.0
        assert np.isnan(out["depth_sigma_c_sq"][i]) and not out["has_mu_app"][i] and out["kappa_app"][i] == 0.0
    # the colour at the clamped, rounded pixel, valid depth or not (:611-616)
    want = np.array([rgb[8, 7], rgb[3, 7], rgb[3, 6], rgb[4, 0], rgb[4, 0], rgb[15, 3], rgb[15, 3]]) / 255.0
    assert np.array_equal(out["color"], want) and out["has_color"].all()
    assert np.array_equal(RS.round_half_away([0.5, 1.5, 2.5, -0.5, -1.5, 0.49999999999999994, -0.4]),
                          [1.0, 2.0, 3.0, -1.0, -2.0, 0.0, -0.0])


def test_restatement_median_and_hex_by_hand():
    depth = np.zeros((9, 9), np.float32)
    depth[3:6, 3:6] = np.array([[2.0, 9.0, 3.0], [np.nan, 5.0, 1.0], [7.0, -1.0, 4.0]], np.float32)
    out = RS.lift(depth, None, [[4.0, 4.0, 1.0]], (10.0, 10.0, 4.0, 4.0), VisualFeatureConfig(quad_fit_min_points=8))
    vals = np.array([2.0, 9.0, 3.0, 5.0, 1.0, 7.0, 4.0])
    assert out["n_window"][0] == 7 and out["z_m"][0] == np.sort(vals)[7 // 2] == 4.0
    assert out["cond"]["n_fit"][0] == 7 and not out["cond"]["fit"][0]      # fewer than min_points: no fit
    sig_sq = (0.01 + 0.01 * 4.0) ** 2
    base = max(vals.var(), sig_sq)
    q = ((vals - 4.0) ** 2).sum() / (7 * base + 1e-12)
    w = max((3.0 + 1.0) / (3.0 + q), 0.1)
    np.testing.assert_allclose(out["depth_sigma_c_sq"][0], base / w, rtol=1e-14)
    assert out["cond"]["from_window"][0]
    # an even count takes the upper middle (rank size / 2)
    depth[5, 5] = 0.0
    out = RS.lift(depth, None, [[4.0, 4.0, 1.0]], (10.0, 10.0, 4.0, 4.0), VisualFeatureConfig())
    assert out["n_window"][0] == 6 and out["z_m"][0] == 5.0
    # hex of radius 1: the centre and six of the eight neighbours, by libm's cos and sin (:303-312)
    offs = RS.hex_offsets(1)
    assert offs[0] == (0, 0) and len(offs) == 7 and all(max(abs(a), abs(b)) == 1 for a, b in offs[1:])
    assert RS.hex_offsets(0) == offs and RS.hex_offsets(2)[1] == (2, 0) and RS.hex_offsets(3)[4] == (-3, 0)
    depth[3:6, 3:6] = np.arange(1.0, 10.0, dtype=np.float32).reshape(3, 3)
    out = RS.lift(depth, None, [[4.0, 4.0, 1.0]], (10.0, 10.0, 4.0, 4.0),
                  VisualFeatureConfig(depth_sample_mode="hex", hex_radius=1))
    hv = np.array([depth[4 + dy, 4 + dx] for dx, dy in offs], np.float64)
    z_hat = np.sort(hv)[7 // 2]
    mad = np.sort(np.abs(hv - z_hat))[7 // 2]
    assert out["n_window"][0] == 7 and out["z_m"][0] == z_hat
    base = max((1.4826 * mad) ** 2, (0.01 + 0.01 * z_hat) ** 2)
    q = ((hv - z_hat) ** 2).sum() / (7 * base + 1e-12)
    np.testing.assert_allclose(out["depth_sigma_c_sq"][0], base / max(4.0 / (3.0 + q), 0.1), rtol=1e-14)
    # fewer than four hex samples: no depth (:327)
    depth[:] = 0.0
    depth[4, 4] = depth[4, 5] = depth[5, 5] = 2.0
    out = RS.lift(depth, None, [[4.0, 4.0, 1.0]], (10.0, 10.0, 4.0, 4.0),
                  VisualFeatureConfig(depth_sample_mode="hex", hex_radius=1))
    assert not out["cond"]["z_valid"][0] and 1 <= out["n_window"][0] < 4 and np.isnan(out["z_m"][0])


@pytest.mark.parametrize("name", list(FC.CASES))
def test_cases_pin_an_implementation(name):
    case = FC.build(name)
    ref, c, cfg = case["ref"], case["ref"]["cond"], case["cfg"]
    m = ref["u"].shape[0]
    assert m == min(FC.CASES[name]["m"], cfg.max_features)
    fit = c["fit"]
    assert fit.any()
    # at most 5 % of the fitted features are left to the solver or to a near-singular H_uv
    with np.errstate(invalid="ignore"):
        ill = float(np.mean(c["cond"][fit] >= 1e6))
        flat = float(np.mean(c["det_ratio"][fit] < 1e-4))
    print(name, "cond >= 1e6: %.3g, |det H|/|H|_F^2 < 1e-4: %.3g of %d fitted" % (ill, flat, int(fit.sum())))
    assert ill <= 0.05 and flat <= 0.05
    assert np.array_equal(ref["has_mu_app"], fit)
    if name == "unsaturated":
        k = c["kappa_clamped"][fit]
        assert np.mean((k > cfg.kappa_min) & (k < cfg.kappa_max)) >= 0.5
    if name == "smallest":
        return
    kinds = {"out of image": ~c["in_image"], "no valid depth": c["in_image"] & ~c["z_valid"],
             "valid depth without a fit": c["z_valid"] & ~fit, "fitted": fit,
             "variance from the model": c["z_valid"] & ~c["from_window"]}
    if cfg.depth_sample_mode == "nearest":
        # the node keeps no window there (:240-244): the variance is the model's on every row
        assert not c["from_window"].any()
    else:
        kinds["variance from the window"] = c["from_window"]
    for kind, rows in kinds.items():
        assert rows.any(), (name, kind)
    assert (ref["weight"][c["z_valid"]] > 0.0).any() and (ref["weight"] == 0.0).any()
    if cfg.depth_sample_mode in ("median3", "median5"):
        r = 1 if cfg.depth_sample_mode == "median3" else 2
        assert (c["n_window"] == (2 * r + 1) ** 2).any() and (c["n_window"][c["z_valid"]] < 4).any()


def test_case_windows_are_what_they_say():
    depth = FC.depth_image()
    ok = np.isfinite(depth) & (depth > 0.0)
    for count, (x, y) in FC.COUNT_SPOTS.items():
        assert ok[y - 1:y + 2, x - 1:x + 2].sum() == count
    for (x, y), r in ((FC.SPARSE_R2, 2), (FC.SPARSE_R3, 3)):
        assert ok[y - 3:y + 4, x - 3:x + 4].sum() == 5 and ok[y, x]
        assert sum(bool(ok[y + dy, x + dx]) for dx, dy in RS.hex_offsets(r)) == 5
    x0, y0 = FC.DEAD_BLOCK
    assert not ok[y0:y0 + 8, x0:x0 + 8].any()
    assert 0.04 < 1.0 - ok.mean() < 0.10
    for bad in (0.0, -1.0):
        assert (depth == bad).any()
    assert np.isnan(depth).any() and np.isposinf(depth).any()
    # the hand-placed rows of the default case are of the kinds they were placed for
    c = FC.build("median3")["ref"]["cond"]
    assert c["n_window"][8:11].tolist() == [1, 3, 4] and c["z_valid"][8:11].all()
    assert c["from_window"][8:11].tolist()[:2] == [False, False]
    assert c["in_image"][2] and not c["in_image"][3] and c["in_image"][4:8].all()
    assert c["z_valid"][11] and not c["fit"][11] and c["in_image"][13] and not c["z_valid"][13]


def test_select_keypoints():
    r = np.array([5.0, 9.0, 5.0, 1.0, 5.0, 7.0, 5.0])
    assert select_keypoints(r, 7).tolist() == list(range(7)) and select_keypoints(r, 10).tolist() == list(range(7))
    assert select_keypoints(r, 2).tolist() == [1, 5]
    assert select_keypoints(r, 3).tolist() == [0, 1, 5]          # the tie at the cut goes to the lower index
    assert select_keypoints(r, 4).tolist() == [0, 1, 2, 5]
    assert select_keypoints(r, 6).tolist() == [0, 1, 2, 4, 5, 6]
    assert select_keypoints(r, 0).tolist() == [] and select_keypoints([], 3).tolist() == []
    assert select_keypoints(r, 3).dtype == np.int64
    for bad in (-1, 2.5):
        with pytest.raises(ValueError):
            select_keypoints(r, bad)
    with pytest.raises(ValueError):
        select_keypoints([1.0, np.nan], 1)
    case = FC.build("truncate")
    assert case["kp"].shape[0] == 80 and case["kept"].shape[0] == 64 and (np.diff(case["kept"]) > 0).all()
    dropped = np.setdiff1d(np.arange(80), case["kept"])
    assert case["kp"][dropped, 2].max() <= case["kp"][case["kept"], 2].min()


def test_config_is_the_nodes():
    cfg = VisualFeatureConfig()
    h = CF._cfg(cfg)
    assert len(h._fields_) == 24 and _abi.GC_CAMFEAT_AUX == 6 == len(CF.AUX_NAMES)
    # visual_feature_node.cpp:74-101 / config/gc_unified.yaml:107-132
    assert [getattr(h, name) for name, _ in h._fields_] == [
        1.0, 1.0, 0.0, 0.01, 0.01, 0.05, 80.0, 5.0, 50.0, 1.0, 1e-9, 1e6, 2.0, 2.0, 6.0, 1e-8, 3.0, 0.1, 10.0, 1e-4, 1.0,
        10.0, 100.0, 0.1]
    assert cfg.max_features == 512
    h = CF._cfg(VisualFeatureConfig(depth_sample_mode="hex", depth_model="quadratic"))
    assert [h.depth_sample_mode, h.depth_model] == [3, 1]
    with pytest.raises(Exception):
        cfg.kappa0 = 2.0  # frozen
    h = CF._cfg(VisualFeatureConfig(hex_radius=0, quad_fit_radius=-4))
    assert [h.hex_radius, h.quad_fit_radius] == [0.0, -4.0]


def _args(**kw):
    a = dict(depth=np.full((6, 8), 2.0, np.float32), rgb=np.zeros((6, 8, 3), np.uint8),
             keypoints_uv=np.array([[3.0, 2.0], [4.0, 4.0]]), responses=np.array([10.0, 20.0]),
             intrinsics=PinholeIntrinsics(10.0, 10.0, 4.0, 3.0), config=VisualFeatureConfig())
    a.update(kw)
    return a


BAD = {
    "too many keypoints": _args(keypoints_uv=np.zeros((4097, 2)), responses=np.ones(4097),
                                config=VisualFeatureConfig(max_features=5000)),
    "empty image": _args(depth=np.zeros((0, 8), np.float32), rgb=None),
    "image over the cap": _args(depth=np.broadcast_to(np.float32(1.0), (8193, 8192)), rgb=None),
    "depth not 2-D": _args(depth=np.zeros((6, 8, 1), np.float32)),
    "depth not numeric": _args(depth=np.full((6, 8), "a")),
    "rgb shape": _args(rgb=np.zeros((6, 7, 3), np.uint8)),
    "rgb channels": _args(rgb=np.zeros((6, 8), np.uint8)),
    "rgb dtype": _args(rgb=np.zeros((6, 8, 3), np.float32)),
    "hex_radius 4": _args(config=VisualFeatureConfig(hex_radius=4)),
    "quad_fit_radius 4": _args(config=VisualFeatureConfig(quad_fit_radius=4)),
    "quad_fit_radius 1.5": _args(config=VisualFeatureConfig(quad_fit_radius=1.5)),
    "quad_fit_min_points 0": _args(config=VisualFeatureConfig(quad_fit_min_points=0)),
    "quad_fit_min_points 2.5": _args(config=VisualFeatureConfig(quad_fit_min_points=2.5)),
    "unknown mode": _args(config=VisualFeatureConfig(depth_sample_mode="median7")),
    "unknown model": _args(config=VisualFeatureConfig(depth_model="cubic")),
    "NaN in the configuration": _args(config=VisualFeatureConfig(kappa_alpha=float("nan"))),
    "max_features": _args(config=VisualFeatureConfig(max_features=-1)),
    "fx 0": _args(intrinsics=PinholeIntrinsics(0.0, 10.0, 4.0, 3.0)),
    "fy 0": _args(intrinsics=(10.0, 0.0, 4.0, 3.0)),
    "cx inf": _args(intrinsics=PinholeIntrinsics(10.0, 10.0, float("inf"), 3.0)),
    "cy NaN": _args(intrinsics=PinholeIntrinsics(10.0, 10.0, 4.0, float("nan"))),
    "three intrinsics": _args(intrinsics=(10.0, 10.0, 4.0)),
    "NaN u": _args(keypoints_uv=np.array([[np.nan, 2.0], [4.0, 4.0]])),
    "inf v": _args(keypoints_uv=np.array([[3.0, np.inf], [4.0, 4.0]])),
    "NaN response": _args(responses=np.array([10.0, np.nan])),
    "keypoint rows": _args(keypoints_uv=np.zeros((2, 3))),
    "response count": _args(responses=np.ones(3)),
}


@pytest.mark.parametrize("what", list(BAD))
def test_argument_errors_need_no_device(what, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(_abi, "default_context", no_device)
    monkeypatch.setattr(_abi, "Context", no_device)
    with pytest.raises(ValueError):
        lift_camera_features(**BAD[what])


def test_no_keypoints_need_no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(_abi, "default_context", no_device)
    for device_out in (False, True):
        for cfg, kp, resp in ((VisualFeatureConfig(), np.zeros((0, 2)), np.zeros(0)),
                              (VisualFeatureConfig(max_features=0), np.ones((3, 2)), np.ones(3))):
            f = lift_camera_features(np.ones((6, 8), np.float32), None, kp, resp, (10.0, 10.0, 4.0, 3.0), cfg,
                                     device_out=device_out)
            assert isinstance(f, CameraFeatures) and len(f) == 0
            assert f.mu_app.shape == (0, 3) and f.cov_xyz.shape == (0, 3, 3) and f.aux.shape == (0, 6)
            assert f.has_mu_app.dtype == bool and f.has_color.dtype == bool
    # the argument checks still run
    with pytest.raises(ValueError):
        lift_camera_features(np.ones((6, 8), np.float32), None, np.zeros((0, 2)), np.zeros(0), (0.0, 10.0, 4.0, 3.0))
