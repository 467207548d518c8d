"""The camera-feature lift on the device (gc_camfeat.hip, gcslam/ops/camera_features.py) against the
restatement (tests/camfeat_restatement.py; parity unpinned by reference vectors, see its header). The
conditions under which the cases pin an implementation are asserted in test_camera_features.py.

Compared exactly: uv, has_mu_app, has_color, color, z_m and with it xyz[:, 2], the window and fit
counts, the rows with weight 0 and with Lambda_c 0, and every row without a valid depth bit for bit.
Every other float array of the valid rows at 1e-10 of the restatement array's max-abs over the valid
rows (the bar of the surfel, VisualPoseEvidence and camera-splat operators). What depends on the fit's
solve (mu_app, kappa_app, the MA term of cov_xyz, lam_min, K) is compared on the rows with
cond(AᵀA + εI) < 1e6 and |det H_uv| / ‖H_uv‖_F² >= 1e-4 (camfeat_restatement.determined) and must be
finite on the others. The measured fractions of the bar are printed by test_gpu_camfeat_parity and
recorded in DESIGN.md §4."""

import ctypes

import numpy as np
import pytest

import camfeat_cases as FC
import camfeat_restatement as RS
from gcslam import _abi
from gcslam.measurement_batch import BATCH_ARRAYS
from gcslam.ops import (CameraFeatures, DeviceCameraFeatures, PinholeIntrinsics, SurfelExtractionConfig,
                        VisualFeatureConfig, camera_measurement_batch, extract_lidar_surfels, lift_camera_features)
from gcslam.ops import camera_features as CF
from gcslam.ops.camera_features import AUX_NAMES

BAR = 1e-10
INTR = PinholeIntrinsics(*FC.K)
FIELDS = ("u", "v", "depth_Lambda_c", "depth_theta_c", "weight", "kappa_app", "mu_app", "has_mu_app", "color",
          "has_color", "xyz", "cov_xyz", "aux")


def _lift(on, case, **kw):
    a = dict(depth=case["depth"], rgb=case["rgb"], keypoints_uv=case["kp"][:, :2], responses=case["kp"][:, 2],
             intrinsics=INTR, config=case["cfg"], ctx=on)
    a.update(kw)
    return lift_camera_features(**a)


def _same_bytes(a: CameraFeatures, b: CameraFeatures):
    for k in FIELDS:
        x, y = np.asarray(getattr(a, k)), np.asarray(getattr(b, k))
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


def _check(f: CameraFeatures, ref, worst):
    """f against a camfeat_restatement.lift result; the worst fraction of the bar per field into worst."""
    c = ref["cond"]
    m = ref["u"].shape[0]
    valid, fit, det = c["z_valid"], c["fit"], RS.determined(c)
    assert isinstance(f, CameraFeatures) and len(f) == m and f.aux.shape == (m, len(AUX_NAMES))
    aux = dict(zip(AUX_NAMES, f.aux.T))
    for k in ("u", "v", "color"):
        assert getattr(f, k).dtype == np.float64 and getattr(f, k).tobytes() == ref[k].tobytes(), k
    for k in ("has_mu_app", "has_color"):
        assert getattr(f, k).dtype == bool and np.array_equal(getattr(f, k), ref[k]), k
    np.testing.assert_array_equal(aux["z_m"], ref["z_m"])       # NaN in the same places
    np.testing.assert_array_equal(f.xyz[:, 2], np.where(valid, ref["z_m"], 0.0))
    np.testing.assert_array_equal(aux["n_window"], ref["n_window"])
    np.testing.assert_array_equal(aux["n_fit"], ref["n_fit"])
    np.testing.assert_array_equal(f.weight == 0.0, ref["weight"] == 0.0)
    np.testing.assert_array_equal(f.depth_Lambda_c == 0.0, ref["depth_Lambda_c"] == 0.0)
    # the rows without a valid depth, bit for bit (:574-575, :602-604)
    inv = ~valid
    for k in ("xyz", "cov_xyz", "weight", "depth_Lambda_c", "depth_theta_c", "kappa_app", "mu_app"):
        assert getattr(f, k)[inv].tobytes() == ref[k][inv].tobytes(), k
    for k in ("depth_sigma_c_sq", "lam_min", "K"):
        assert aux[k][inv].tobytes() == ref[k][inv].tobytes(), k
    assert np.isnan(aux["depth_sigma_c_sq"][inv]).all()
    got = dict(depth_Lambda_c=f.depth_Lambda_c, depth_theta_c=f.depth_theta_c, weight=f.weight, kappa_app=f.kappa_app,
               mu_app=f.mu_app, xyz=f.xyz, cov_xyz=f.cov_xyz, depth_sigma_c_sq=aux["depth_sigma_c_sq"],
               lam_min=aux["lam_min"], K=aux["K"])
    pinned = valid & (~fit | det)
    for k in RS.FLOAT_KEYS:
        rows = pinned if k in RS.FIT_KEYS else valid
        worst[k] = max(worst.get(k, 0.0), FC.err_frac(got[k], ref[k], BAR, rows, valid))
        assert np.isfinite(got[k][valid]).all(), k              # the rows the solve leaves open: finite
    # without a fit nothing depends on a solve: no mu_app, no kappa, no MA term
    nofit = valid & ~fit
    assert not f.mu_app[nofit].any() and not f.kappa_app[nofit].any() and not aux["K"][nofit].any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FC.CASES))
def test_gpu_camfeat_parity(ctx, name):
    case = FC.build(name)
    worst = {}
    _check(_lift(ctx, case), case["ref"], worst)
    print(name, "fraction of the 1e-10 bar:", {k: float("%.3g" % v) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.gpu
def test_gpu_camfeat_reproducible(ctx):
    case = FC.build("median3")
    a, b = _lift(ctx, case), _lift(ctx, case)
    _same_bytes(a, b)
    assert a.has_mu_app.any() and np.isfinite(a.kappa_app).all()


@pytest.mark.gpu
def test_gpu_camfeat_device_inputs(ctx):
    """depth and rgb as DeviceArrays give the bytes host arrays give; a host depth of another dtype is
    converted to float32 first; device_out keeps every array in HBM."""
    case = FC.build("hex")
    host = _lift(ctx, case)
    d_depth = _abi.DeviceArray.from_host(ctx, case["depth"], np.float32)
    d_rgb = _abi.DeviceArray.from_host(ctx, case["rgb"], np.uint8)
    _same_bytes(host, _lift(ctx, case, depth=d_depth, rgb=d_rgb))
    _same_bytes(host, _lift(ctx, case, depth=d_depth, rgb=d_rgb, ctx=None))   # the arrays' own context
    _same_bytes(host, _lift(ctx, case, depth=case["depth"].astype(np.float64)))
    dev = _lift(ctx, case, device_out=True)
    assert isinstance(dev, DeviceCameraFeatures) and len(dev) == len(host)
    assert all(isinstance(getattr(dev, k), _abi.DeviceArray) for k in FIELDS[2:] + ("uv",))
    assert dev.uv.shape == (len(host), 2) and dev.has_mu_app.dtype == np.uint8 and dev.aux.shape == host.aux.shape
    assert dev.u.tobytes() == host.u.tobytes() and dev.v.tobytes() == host.v.tobytes()
    _same_bytes(host, dev.to_host())
    with pytest.raises(ValueError):
        _lift(ctx, case, depth=_abi.DeviceArray.from_host(ctx, case["depth"].astype(np.float64)))
    # a 16-bit millimetre image with depth_scale = 1e-3
    live = np.isfinite(case["depth"]) & (case["depth"] > 0)
    ints = np.round(np.where(live, case["depth"], 0.0) * 1000.0).astype(np.uint16)
    cfg = VisualFeatureConfig(depth_scale=0.001)
    a = _lift(ctx, case, depth=ints, config=cfg)
    _same_bytes(a, _lift(ctx, case, depth=ints.astype(np.float32), config=cfg))
    worst = {}
    _check(a, RS.lift(ints.astype(np.float32), case["rgb"], case["kp"], FC.K, cfg), worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.gpu
def test_gpu_camfeat_device_chain(ctx):
    """lift_camera_features(device_out) -> camera_measurement_batch(DeviceCameraFeatures, device_out) ->
    extract_lidar_surfels(base_batch), nothing returning to the host between them, gives the bytes of
    the same chain through a host download and a host CameraFeatures."""
    import camsplat_cases as CC
    import surfel_cases as SC
    case = FC.build("median3")
    points = CC.build("mixed")["points_base"]
    s = SC.build("overflow_truncate")
    scfg = SurfelExtractionConfig(**dict(s["cfg"], n_feat=64))
    assert scfg.n_surfel == 64

    def chain(features):
        cam = camera_measurement_batch(points, features, INTR, CC.R_BASE_CAMERA, CC.T_BASE_CAMERA, CC.TIMESTAMP,
                                       n_feat=64, n_surfel=64, eps_lift=CC.EPS_LIFT, ctx=ctx, device_out=True)
        full, _, _ = extract_lidar_surfels(s["points"], s["timestamps"], s["weights"], scfg, base_batch=cam, ctx=ctx,
                                           device_out=True)
        return cam, full

    dev = _lift(ctx, case, device_out=True)
    cam_a, full_a = chain(dev)
    host = _lift(ctx, case)
    assert isinstance(host, CameraFeatures) and not isinstance(host, DeviceCameraFeatures)
    cam_b, full_b = chain(host)
    assert (full_a.n_camera_valid, full_a.n_lidar_valid) == (full_b.n_camera_valid, full_b.n_lidar_valid)
    assert full_a.n_camera_valid == 64 and full_a.n_lidar_valid > 0
    for batch_a, batch_b in ((cam_a, cam_b), (full_a, full_b)):
        for k in BATCH_ARRAYS:
            x, y = batch_a.device[k].download(), batch_b.device[k].download()
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
    # the camera rows carry the lift: weights, colours and the vMF lobe kappa_app * direction
    w = cam_a.device["weights"].download()[:64]
    assert w.tobytes() == host.weight.tobytes()
    col = cam_a.device["colors"].download()[:64]
    assert np.array_equal(col, np.clip(host.color, 0.0, 1.0))
    eta = cam_a.device["etas"].download()[:64, 0]
    np.testing.assert_allclose(np.linalg.norm(eta, axis=1), host.kappa_app, rtol=1e-9, atol=1e-12)
    # the diagnostics of the fused call for device features
    _, diag = camera_measurement_batch(points, dev, INTR, CC.R_BASE_CAMERA, CC.T_BASE_CAMERA, CC.TIMESTAMP, n_feat=64,
                                       n_surfel=64, eps_lift=CC.EPS_LIFT, ctx=ctx, return_diag=True)
    _, diag_b = camera_measurement_batch(points, host, INTR, CC.R_BASE_CAMERA, CC.T_BASE_CAMERA, CC.TIMESTAMP,
                                         n_feat=64, n_surfel=64, eps_lift=CC.EPS_LIFT, ctx=ctx, return_diag=True)
    assert diag.xyz.tobytes() == diag_b.xyz.tobytes() and diag.fused.tobytes() == diag_b.fused.tobytes()
    assert diag.fused.any()


def _raw_call(ctx, H=4, W=4, depth=1, M=0, intr=(10.0, 10.0, 2.0, 2.0), cfg=None):
    """gc_camera_features_lift itself with M = 0 (no buffer is touched): the entry's own argument checks."""
    h_k = np.array(intr, np.float64)
    c_cfg = CF._cfg(VisualFeatureConfig())
    for name, v in (cfg or {}).items():
        getattr(c_cfg, name)  # a member of gc_camfeat_cfg
        setattr(c_cfg, name, v)
    buf = _abi.DeviceArray(ctx, (16,), np.float32)
    _abi.call("gc_camera_features_lift", ctx.handle, H, W, buf.ptr if depth else None, None, M, None, h_k.ctypes.data,
              ctypes.byref(c_cfg), *([None] * 12), ctx=ctx)


@pytest.mark.gpu
def test_gpu_camfeat_edges(ctx):
    case = FC.build("median3")
    # M = 0
    f = _lift(ctx, case, keypoints_uv=np.zeros((0, 2)), responses=np.zeros(0))
    assert isinstance(f, CameraFeatures) and len(f) == 0 and f.cov_xyz.shape == (0, 3, 3)
    # rgb = None: no colours, everything else the same bytes
    a, b = _lift(ctx, case), _lift(ctx, case, rgb=None)
    assert a.has_color.all() and a.color.any() and not b.has_color.any() and not b.color.any()
    for k in FIELDS:
        if k not in ("color", "has_color"):
            assert np.asarray(getattr(a, k)).tobytes() == np.asarray(getattr(b, k)).tobytes(), k
    # a 1 x 1 image: one value to take the median of, nothing to fit
    one = np.array([[2.5]], np.float32)
    px = np.array([[7, 9, 11]], np.uint8).reshape(1, 1, 3)
    kp = np.array([[0.0, 0.0, 30.0], [0.4, -0.3, 30.0], [0.5, 0.0, 30.0], [0.0, -0.5, 30.0], [-0.49, 0.49, 0.0]])
    for mode in ("nearest", "median3", "median5", "hex"):
        cfg = VisualFeatureConfig(depth_sample_mode=mode)
        f = lift_camera_features(one, px, kp[:, :2], kp[:, 2], (1.0, 1.0, 0.0, 0.0), cfg, ctx=ctx)
        ref = RS.lift(one, px, kp, (1.0, 1.0, 0.0, 0.0), cfg)
        worst = {}
        _check(f, ref, worst)
        assert max(worst.values()) <= 1.0, (mode, worst)
        want_valid = [mode != "hex", mode != "hex", False, False, mode != "hex"]
        assert ref["cond"]["z_valid"].tolist() == want_valid and not f.has_mu_app.any()
        assert np.array_equal(f.color, np.tile(px.reshape(1, 3) / 255.0, (5, 1)))
    # every keypoint outside the image: every row the invalid row
    out = np.array([[-3.0, 5.0, 9.0], [FC.W + 0.5, 5.0, 9.0], [5.0, -0.5, 9.0], [5.0, FC.H - 0.5, 9.0], [-1e9, 1e12, 9.0]])
    f = _lift(ctx, case, keypoints_uv=out[:, :2], responses=out[:, 2])
    ref = RS.lift(case["depth"], case["rgb"], out, FC.K, case["cfg"])
    assert not ref["cond"]["in_image"].any()
    worst = {}
    _check(f, ref, worst)
    assert np.array_equal(f.cov_xyz, np.tile(np.eye(3) * 1e6, (5, 1, 1))) and not f.xyz.any() and not f.weight.any()
    assert f.has_color.all() and np.array_equal(f.color[0], case["rgb"][5, 0] / 255.0)
    # H W over the cap: refused before anything is uploaded
    with pytest.raises(ValueError):
        _lift(ctx, case, depth=np.broadcast_to(np.float32(1.0), (8192, 8193)), rgb=None)
    # the entry's own checks, before any launch
    _raw_call(ctx)
    _raw_call(ctx, cfg=dict(hex_radius=0))       # max(1, r) first
    _raw_call(ctx, cfg=dict(quad_fit_radius=-7))
    _raw_call(ctx, H=8192, W=8192)
    for bad in (dict(M=-1), dict(M=4097), dict(H=0), dict(W=0), dict(H=8192, W=8193), dict(depth=0),
                dict(cfg=dict(hex_radius=4)), dict(cfg=dict(quad_fit_radius=4)), dict(cfg=dict(quad_fit_radius=2.5)),
                dict(cfg=dict(quad_fit_min_points=0)), dict(cfg=dict(depth_sample_mode=4)),
                dict(cfg=dict(depth_sample_mode=1.5)), dict(cfg=dict(depth_model=2)), dict(cfg=dict(kappa_alpha=float("nan"))),
                dict(intr=(0.0, 10.0, 2.0, 2.0)), dict(intr=(10.0, 0.0, 2.0, 2.0)),
                dict(intr=(10.0, 10.0, float("inf"), 2.0)), dict(intr=(10.0, 10.0, 2.0, float("nan")))):
        with pytest.raises(ValueError):
            _raw_call(ctx, **bad)
    # NULL output pointers with keypoints to lift
    with pytest.raises(ValueError):
        _raw_call(ctx, M=1)
    _same_bytes(a, _lift(ctx, case))       # the context stays usable
