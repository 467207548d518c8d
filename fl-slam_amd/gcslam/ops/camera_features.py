"""The image side of the camera features on the GPU: what the reference's visual_feature_node
(src/visual_feature_node.cpp:493-652) computes per ORB keypoint from the depth and the colour image,
and what the backend makes of its message (backend/backend_node.py:1589-1645), as the CameraFeatures
camera_measurement_batch takes. Per keypoint: a robust depth sample (:228-348), the Student-t
variance inflation (:350-369), the quadratic surface fit with its normal, Gaussian curvature and
smaller Hessian eigenvalue (:401-491), the closed-form backprojection covariance (:371-399), the vMF
concentration, the depth natural parameters and the colour (:547-634). Keypoints (u, v, response) are
the input, as the LiDAR points are the surfel extractor's: the caller's own detector's on the host, or
the table detect_keypoints (keypoint_detector.py) leaves in HBM.
All arithmetic runs in libgcslam (csrc/gc_camfeat.hip); every argument error is raised here before a
device is asked for."""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .. import _abi
from .camera_splats import CameraFeatures, DeviceCameraFeatures, PinholeIntrinsics, _intr_vector, _n_rows
from .keypoint_detector import DeviceKeypoints

DEPTH_SAMPLE_MODES = ("nearest", "median3", "median5", "hex")  # the codes 0..3 of gc_camfeat_cfg.depth_sample_mode
DEPTH_MODELS = ("linear", "quadratic")                         # the codes 0, 1
AUX_NAMES = ("depth_sigma_c_sq", "z_m", "n_window", "n_fit", "lam_min", "K")  # the columns of aux
MAX_RADIUS = _abi.GC_CAMFEAT_MAX_RADIUS  # gc_camfeat.hip: one lane per window pixel, (2 r + 1)^2 <= 64
MAX_PIXELS = _abi.GC_IMAGE_MAX_PIXELS


@dataclass(frozen=True)
class VisualFeatureConfig:
    """visual_feature_node.cpp:70, :74-101: the node's parameters and defaults (those of
    config/gc_unified.yaml:107-132, there with the prefix visual_feature_). The fields after
    max_features are the members of gc_camfeat_cfg (include/gcslam.h) under the same names. cov_reg_eps is
    declared by the node and never read."""
    max_features: int = 512
    depth_sample_mode: str = "median3"
    pixel_sigma: float = 1.0
    depth_model: str = "linear"
    depth_sigma0: float = 0.01
    depth_sigma_slope: float = 0.01
    min_depth_m: float = 0.05
    max_depth_m: float = 80.0
    depth_validity_slope: float = 5.0
    response_soft_scale: float = 50.0
    depth_scale: float = 1.0
    cov_reg_eps: float = 1e-9
    invalid_cov_inflate: float = 1e6
    hex_radius: int = 2
    quad_fit_radius: int = 2
    quad_fit_min_points: int = 6
    quad_fit_lstsq_eps: float = 1e-8
    student_t_nu: float = 3.0
    student_t_w_min: float = 0.1
    ma_tau: float = 10.0
    ma_delta_inflate: float = 1e-4
    kappa0: float = 1.0
    kappa_alpha: float = 10.0
    kappa_max: float = 100.0
    kappa_min: float = 0.1


def _cfg(cfg: VisualFeatureConfig):
    """gc_camfeat_cfg (include/gcslam.h), checked as the device entry checks it."""
    if cfg.depth_sample_mode not in DEPTH_SAMPLE_MODES:  # the node throws (:256)
        raise ValueError(f"Unknown depth_sample_mode: {cfg.depth_sample_mode!r}; one of {DEPTH_SAMPLE_MODES}")
    if cfg.depth_model not in DEPTH_MODELS:  # :225
        raise ValueError(f"Unknown depth_model: {cfg.depth_model!r}; one of {DEPTH_MODELS}")
    try:
        h = _abi.cfg("gc_camfeat_cfg", cfg, depth_sample_mode=DEPTH_SAMPLE_MODES.index(cfg.depth_sample_mode),
                     depth_model=DEPTH_MODELS.index(cfg.depth_model))
    except (TypeError, ValueError) as e:
        raise ValueError(f"config does not hold the VisualFeatureConfig fields: {e}") from None
    if np.isnan(np.frombuffer(h, np.float64)).any():
        raise ValueError("NaN in the configuration")
    for name in ("hex_radius", "quad_fit_radius"):
        r = getattr(cfg, name)
        if not math.isfinite(r) or int(r) != r or max(1, int(r)) > MAX_RADIUS:  # the node's max(1, r) first
            raise ValueError(f"{name} must be an integer with max(1, {name}) in [1, {MAX_RADIUS}], got {r}")
    mp = cfg.quad_fit_min_points
    if not math.isfinite(mp) or int(mp) != mp or not 1 <= mp <= 1 << 24:
        raise ValueError(f"quad_fit_min_points must be an integer >= 1, got {mp}")
    return h


def _max_features(cfg: VisualFeatureConfig) -> int:
    k = cfg.max_features
    if isinstance(k, float) and not math.isfinite(k) or int(k) != k or k < 0:
        raise ValueError(f"max_features must be an integer >= 0, got {k}")
    return int(k)


def select_keypoints(responses, max_features: int) -> np.ndarray:
    """The keypoints the node keeps when the detector returns more than max_features (:523-535): the
    indices of the max_features largest responses, ties at the cut going to the lower index, in input
    (ascending index) order. The node's own order inside the kept set, and which of several equal
    responses at the cut it keeps, are std::nth_element's and unspecified; the set is the same wherever
    the responses at the cut differ. Host code."""
    r = np.asarray(responses, dtype=np.float64).reshape(-1)
    if np.isnan(r).any():
        raise ValueError("NaN response")
    if int(max_features) != max_features or max_features < 0:
        raise ValueError(f"max_features must be an integer >= 0, got {max_features}")
    k = int(max_features)
    if r.shape[0] <= k:
        return np.arange(r.shape[0], dtype=np.int64)
    order = np.lexsort((np.arange(r.shape[0]), -r))  # by descending response, then ascending index
    return np.sort(order[:k]).astype(np.int64)


def image_shape(x, what: str, channels: Optional[int]):
    sh = tuple(int(v) for v in (x.shape if isinstance(x, _abi.DeviceArray) else np.shape(x)))
    want = 2 if channels is None else 3
    if len(sh) != want or (channels is not None and sh[2] != channels):
        raise ValueError(f"{what} of shape {sh}, expected (H, W{'' if channels is None else ', %d' % channels})")
    return sh


def depth_image(depth, what: str):
    """(H, W, image) of a depth image called `what`: the float32 DeviceArray itself, or the host image as
    contiguous float32 (another float or integer dtype is converted)."""
    H, W = image_shape(depth, what, None)
    if isinstance(depth, _abi.DeviceArray):
        if depth.dtype != np.float32:
            raise ValueError(f"device {what} of dtype {depth.dtype}, expected float32")
        return H, W, depth
    depth = np.asarray(depth)
    if depth.dtype.kind not in "fiu":
        raise ValueError(f"{what} of dtype {depth.dtype}, expected a float or integer image")
    return H, W, np.ascontiguousarray(depth, dtype=np.float32)


def _empty(m: int = 0) -> CameraFeatures:
    z = lambda *s: np.zeros((m,) + s, np.float64)
    return CameraFeatures(u=z(), v=z(), depth_Lambda_c=z(), depth_theta_c=z(), weight=z(), kappa_app=z(), mu_app=z(3),
                          has_mu_app=np.zeros(m, bool), color=z(3), has_color=np.zeros(m, bool), xyz=z(3),
                          cov_xyz=z(3, 3), aux=z(_abi.GC_CAMFEAT_AUX))


_OUT = (("uv", (2,), np.float64), ("depth_Lambda_c", (), np.float64), ("depth_theta_c", (), np.float64),
        ("weight", (), np.float64), ("kappa_app", (), np.float64), ("mu_app", (3,), np.float64),
        ("has_mu_app", (), np.uint8), ("color", (3,), np.float64), ("has_color", (), np.uint8),
        ("xyz", (3,), np.float64), ("cov_xyz", (3, 3), np.float64), ("aux", (_abi.GC_CAMFEAT_AUX,), np.float64))


def lift_camera_features(depth, rgb, keypoints_uv, responses, intrinsics,
                         config: Optional[VisualFeatureConfig] = None, *, ctx=None, device_out: bool = False):
    """visual_feature_node.cpp:537-641 without the detector, and _feature_batch_to_list
    (backend_node.py:1589-1645): the CameraFeatures of M keypoints. depth (H, W) in metres before
    depth_scale and rgb (H, W, 3) uint8 or None (no colours: has_color False, color 0) are host arrays
    or DeviceArrays (float32 / uint8); a host depth of another float or integer dtype is converted to
    float32 first (the node always receives 32FC1). keypoints_uv (M, 2) and responses (M) are host
    arrays; more than config.max_features of them are cut with select_keypoints first. keypoints_uv may
    instead be the DeviceKeypoints of detect_keypoints(..., device_out=True) with responses None: the
    first count rows of its (u, v, response) table are read in HBM, and a count above
    config.max_features is a ValueError. intrinsics: a PinholeIntrinsics or [fx, fy, cx, cy].

    Returns CameraFeatures with aux (M, GC_CAMFEAT_AUX; AUX_NAMES) set; with device_out a
    DeviceCameraFeatures whose arrays stay in HBM for camera_measurement_batch. M = 0 returns the empty
    host CameraFeatures in either case, without asking for a device. has_mu_app marks the rows with a
    fit; a keypoint without a valid depth has xyz 0, cov_xyz invalid_cov_inflate I, weight 0,
    depth_Lambda_c = depth_theta_c = 0 and a NaN depth_sigma_c_sq."""
    cfg = config or VisualFeatureConfig()
    c_cfg = _cfg(cfg)
    k_max = _max_features(cfg)
    if isinstance(intrinsics, PinholeIntrinsics):
        intrinsics = (intrinsics.fx, intrinsics.fy, intrinsics.cx, intrinsics.cy)
    try:
        fx, fy, cx, cy = intrinsics
    except (TypeError, ValueError):
        raise ValueError("intrinsics must be a PinholeIntrinsics or [fx, fy, cx, cy]") from None
    h_k = _intr_vector(fx, fy, cx, cy)
    H, W, depth = depth_image(depth, "depth")
    if H < 1 or W < 1 or H * W > MAX_PIXELS:
        raise ValueError(f"a depth image of {H} x {W}; H and W must be >= 1 and H W <= 2^26")
    if rgb is not None:
        rgb_shape = image_shape(rgb, "rgb", 3)
        if rgb_shape[:2] != (H, W):
            raise ValueError(f"rgb of shape {rgb_shape} for a depth image of {H} x {W}")
        if not isinstance(rgb, _abi.DeviceArray):
            rgb = np.asarray(rgb)
        if rgb.dtype != np.uint8:
            raise ValueError(f"rgb of dtype {rgb.dtype}, expected uint8 (rgb8)")
    dev_kp = keypoints_uv if isinstance(keypoints_uv, DeviceKeypoints) else None
    if dev_kp is not None:
        # the detector's table, read where it is: the first count rows, no download and no upload
        if responses is not None:
            raise ValueError("responses must be None with a DeviceKeypoints: its table carries them")
        m = int(dev_kp.count)
        if m > k_max:
            raise ValueError(f"{m} device keypoints for max_features = {k_max}: detect with the same budget")
        if m > dev_kp.table.shape[0] or dev_kp.table.shape[1:] != (3,) or dev_kp.table.dtype != np.float64:
            raise ValueError(f"a DeviceKeypoints table of shape {dev_kp.table.shape} for count = {m}")
    else:
        try:
            uv = np.asarray(keypoints_uv, dtype=np.float64)
            resp = np.asarray(responses, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"keypoints_uv and responses must be numeric arrays: {e}") from None
        if uv.ndim == 1 and uv.size == 2:
            uv = uv.reshape(1, 2)
        m = _n_rows(uv, 2, "keypoints_uv")
        if _n_rows(resp, 1, "responses") != m:
            raise ValueError(f"responses holds {_n_rows(resp, 1, 'responses')} values for {m} keypoints")
        kp = np.concatenate([uv.reshape(m, 2), resp.reshape(m, 1)], axis=1)
        if not np.isfinite(kp).all():
            raise ValueError("u, v and response must be finite")
        if m > k_max:
            kp = kp[select_keypoints(kp[:, 2], k_max)]
            m = kp.shape[0]
    if m > _abi.GC_CAM_MAX_QUERIES:
        raise ValueError(f"{m} keypoints; at most {_abi.GC_CAM_MAX_QUERIES} are supported")
    if m == 0:
        return _empty()
    if ctx is None:
        dev_in = [x for x in (depth, rgb) if isinstance(x, _abi.DeviceArray)]
        ctx = dev_in[0].ctx if dev_in else (dev_kp.table.ctx if dev_kp is not None else _abi.default_context())
    d_depth = _abi.device_input(ctx, depth, np.float32, (H, W))
    d_rgb = _abi.device_input(ctx, rgb, np.uint8, (H, W, 3)) if rgb is not None else None
    if dev_kp is not None:
        d_kp = dev_kp.table
    else:
        (d_kp,) = _abi.upload_many(ctx, [np.ascontiguousarray(kp)])
    out = _abi.alloc_many(ctx, [((m,) + shp, dt) for _, shp, dt in _OUT])
    _abi.call("gc_camera_features_lift", ctx.handle, H, W, d_depth.ptr, d_rgb.ptr if d_rgb is not None else None, m,
              d_kp.ptr, h_k.ctypes.data, C.byref(c_cfg), *[o.ptr for o in out], ctx=ctx)
    dev = DeviceCameraFeatures(**{name: o for (name, _, _), o in zip(_OUT, out)})
    return dev if device_out else dev.to_host()
