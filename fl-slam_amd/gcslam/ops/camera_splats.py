"""Camera splats on the GPU: the camera half of a MeasurementBatch. The reference computes it once
per scan in backend_node.py:1872-1925: the scan's points go to the camera frame, lidar_depth_evidence
(frontend/sensors/lidar_camera_depth_fusion.py:389-442, Route A :99-164 and Route B :242-386) gives
every camera feature a LiDAR depth in natural parameters, splat_prep_fused
(frontend/sensors/splat_prep.py:37-134) fuses it with the camera's own depth and backprojects, every
feature goes back to the base frame, and feature_list_to_camera_batch
(backend/camera_batch_utils.py:23-86) with measurement_batch_from_camera_splats
(backend/structures/measurement_batch.py:165-259) writes rows [0, n_feat). All arithmetic runs in
libgcslam (csrc/gc_camsplat.hip); every argument error is raised here before a device is asked for."""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, fields
from typing import Optional, Sequence

import numpy as np

from .. import _abi
from ..constants import GC_EPS_LIFT, GC_N_FEAT, GC_N_SURFEL, GC_VMF_N_LOBES
from ..measurement_batch import BATCH_ARRAYS, MeasurementBatch, create_empty_measurement_batch


@dataclass(frozen=True)
class LidarCameraDepthFusionConfig:
    """lidar_camera_depth_fusion.py:29-63, the reference's fields and defaults: the members of gc_cam_cfg
    (include/gcslam.h) under the same names."""
    depth_fusion_weight_camera: float = 1.0
    depth_fusion_weight_lidar: float = 1.0
    gamma_lidar: float = 1.0
    lidar_projection_radius_pix: float = 3.0
    lidar_plane_fit_min_points: int = 3
    lidar_depth_base_sigma_m: float = 0.02
    lidar_incidence_sigma_scale: float = 1.0
    depth_var_min_m2: float = 1e-8
    point_support_n0: float = 3.0
    point_support_alpha: float = 1.0
    spread_mad_beta: float = 10.0
    repr_gamma: float = 10.0
    lidar_ray_plane_fit_max_points: int = 64
    plane_intersection_delta: float = 1e-6
    plane_angle_sigmoid_alpha: float = 10.0
    plane_angle_sigmoid_t: float = 0.1
    plane_planarity_sigmoid_beta: float = 5.0
    plane_planarity_rho0: float = 0.3
    plane_residual_exp_gamma: float = 100.0
    plane_fit_eps: float = 1e-12
    depth_min_m: float = 0.05
    depth_sigma_max_sq: float = 1e4
    depth_min_sigmoid_alpha_z: float = 20.0


@dataclass(frozen=True)
class PinholeIntrinsics:
    """frontend/sensors/visual_types.py:16-21."""
    fx: float
    fy: float
    cx: float
    cy: float


@dataclass
class CameraFeatures:
    """The M features of one image as arrays: what splat_prep_fused and the node read of a Feature3D
    (visual_types.py:24-61). depth_Lambda_c / depth_theta_c are meta["depth_Lambda_c"] /
    meta["depth_theta_c"] (0 where absent); mu_app and color are read where has_mu_app / has_color are
    set; xyz and cov_xyz (camera frame) are the feature's own, used where the fusion falls back."""
    u: np.ndarray
    v: np.ndarray
    depth_Lambda_c: np.ndarray
    depth_theta_c: np.ndarray
    weight: np.ndarray
    kappa_app: np.ndarray
    mu_app: np.ndarray         # (M, 3)
    has_mu_app: np.ndarray     # (M,) bool
    color: np.ndarray          # (M, 3)
    has_color: np.ndarray      # (M,) bool
    xyz: np.ndarray            # (M, 3)
    cov_xyz: np.ndarray        # (M, 3, 3)
    aux: Optional[np.ndarray] = None  # (M, GC_CAMFEAT_AUX) from lift_camera_features; nothing here reads it

    def __len__(self) -> int:
        return int(np.shape(self.u)[0])


@dataclass
class DeviceCameraFeatures:
    """CameraFeatures in HBM, as lift_camera_features(..., device_out=True) leaves them: the same
    names holding DeviceArrays laid out as gc_camera_measurement_batch reads them (uv one (M, 2) array,
    the two flags uint8), plus aux (M, GC_CAMFEAT_AUX; camera_features.AUX_NAMES).
    camera_measurement_batch passes the pointers on as they are."""
    uv: "_abi.DeviceArray"
    depth_Lambda_c: "_abi.DeviceArray"
    depth_theta_c: "_abi.DeviceArray"
    weight: "_abi.DeviceArray"
    kappa_app: "_abi.DeviceArray"
    mu_app: "_abi.DeviceArray"
    has_mu_app: "_abi.DeviceArray"
    color: "_abi.DeviceArray"
    has_color: "_abi.DeviceArray"
    xyz: "_abi.DeviceArray"
    cov_xyz: "_abi.DeviceArray"
    aux: "_abi.DeviceArray"

    def __len__(self) -> int:
        return int(self.uv.shape[0])

    @property
    def u(self) -> np.ndarray:
        """Column 0 of uv on the host (a download: the columns are strided in HBM)."""
        return np.ascontiguousarray(self.uv.download()[:, 0])

    @property
    def v(self) -> np.ndarray:
        return np.ascontiguousarray(self.uv.download()[:, 1])

    def to_host(self) -> CameraFeatures:
        """The host CameraFeatures with the same values (one download when the arrays share a block)."""
        names = [f.name for f in fields(self)]
        h = dict(zip(names, _abi.download_many([getattr(self, k) for k in names])))
        uv = h.pop("uv")
        for k in ("has_mu_app", "has_color"):
            h[k] = h[k].astype(bool)
        return CameraFeatures(u=np.ascontiguousarray(uv[:, 0]), v=np.ascontiguousarray(uv[:, 1]),
                              **{k: np.array(a) for k, a in h.items()})


@dataclass
class CameraSplatDiagnostics:
    """What the fused call computed per feature besides the batch: splat_prep_fused's xyz and cov_xyz
    (camera frame), whether the depth was fused (False: the feature's own xyz / cov_xyz), the evidence
    and the number of LiDAR points within the projection radius."""
    xyz: np.ndarray
    cov_xyz: np.ndarray
    fused: np.ndarray
    Lambda_ell: np.ndarray
    theta_ell: np.ndarray
    Lambda_A: np.ndarray
    theta_A: np.ndarray
    Lambda_B: np.ndarray
    theta_B: np.ndarray
    z_B: np.ndarray
    sigma_sq_B: np.ndarray
    w_B: np.ndarray
    n_in_radius: np.ndarray


_EV_NAMES = ("Lambda_A", "theta_A", "Lambda_B", "theta_B", "Lambda_ell", "theta_ell", "z_B", "sigma_sq_B", "w_B")


def _cfg(cfg: LidarCameraDepthFusionConfig):
    """gc_cam_cfg (include/gcslam.h), checked as the device entry checks it."""
    try:
        h = _abi.cfg("gc_cam_cfg", cfg)
    except (TypeError, ValueError) as e:
        raise ValueError(f"config does not hold the LidarCameraDepthFusionConfig fields: {e}") from None
    if np.isnan(np.frombuffer(h, np.float64)).any():
        raise ValueError("NaN in the configuration")
    r = cfg.lidar_projection_radius_pix
    if not (r > 0.0 and math.isfinite(r)):
        raise ValueError(f"lidar_projection_radius_pix must be > 0 and finite, got {r}")
    mp = cfg.lidar_plane_fit_min_points
    if int(mp) != mp or mp < 1:
        raise ValueError(f"lidar_plane_fit_min_points must be an integer >= 1, got {mp}")
    k = cfg.lidar_ray_plane_fit_max_points
    if int(k) != k or not 1 <= k <= _abi.GC_CAM_MAX_FIT_POINTS:
        raise ValueError(f"lidar_ray_plane_fit_max_points must be an integer in [1, {_abi.GC_CAM_MAX_FIT_POINTS}], "
                         f"got {k}")
    return h


def _intr_vector(fx, fy, cx, cy) -> np.ndarray:
    h = np.array([float(fx), float(fy), float(cx), float(cy)], np.float64)
    if not np.isfinite(h).all():
        raise ValueError(f"the intrinsics must be finite, got {h.tolist()}")
    if h[0] == 0.0 or h[1] == 0.0:
        raise ValueError("fx and fy must not be 0")
    return h


def _n_rows(x, width: int, what: str) -> int:
    sh = x.shape if isinstance(x, _abi.DeviceArray) else np.shape(x)
    n = math.prod(int(v) for v in sh) if sh else 1
    if n == 0 and len(sh):
        return 0
    if len(sh) == 0 or n % width or (len(sh) >= 2 and math.prod(int(v) for v in sh[1:]) != width):
        raise ValueError(f"{what} of shape {tuple(sh)} does not hold rows of {width}")
    return n // width


def _check_counts(n: int, m: int) -> None:
    if n > _abi.GC_CAM_MAX_POINTS:
        raise ValueError(f"{n} points; at most {_abi.GC_CAM_MAX_POINTS} (2^22) are supported")
    if m > _abi.GC_CAM_MAX_QUERIES:
        raise ValueError(f"{m} queries; at most {_abi.GC_CAM_MAX_QUERIES} are supported")


def _check_budget(n_feat, n_surfel) -> None:
    if int(n_feat) != n_feat or n_feat < 0 or n_feat > 1 << 24:
        raise ValueError(f"n_feat must be an integer in [0, 2^24], got {n_feat}")
    if int(n_surfel) != n_surfel or n_surfel < 0 or n_surfel > 1 << 24:
        raise ValueError(f"n_surfel must be an integer in [0, 2^24], got {n_surfel}")


def _host_rows(x, shape, what: str) -> np.ndarray:
    try:
        return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(shape))
    except (TypeError, ValueError):
        raise ValueError(f"{what} of shape {np.shape(x)} does not fit {shape}") from None


def lidar_depth_evidence(points_camera_frame, uv_query, fx, fy, cx, cy,
                         config: Optional[LidarCameraDepthFusionConfig] = None, *, point_weights=None,
                         return_diag: bool = False, ctx=None):
    """lidar_camera_depth_fusion.py:389-442: (Lambda_ell, theta_ell) per query pixel, with return_diag
    also a dict with Lambda_A, theta_A, Lambda_B, theta_B (the reference's keys) and z_B, sigma_sq_B,
    w_B, n_in_radius. points_camera_frame (N, 3) may be a DeviceArray. point_weights must hold N values
    (the reference silently ignores another size; here that is an argument error)."""
    cfg = config or LidarCameraDepthFusionConfig()
    c_cfg, h_k = _cfg(cfg), _intr_vector(fx, fy, cx, cy)
    n = _n_rows(points_camera_frame, 3, "points_camera_frame")
    uv = np.asarray(uv_query, dtype=np.float64)
    if uv.ndim == 1 and uv.size == 2:
        uv = uv.reshape(1, 2)
    m = _n_rows(uv, 2, "uv_query")
    _check_counts(n, m)
    if point_weights is not None and _n_rows(point_weights, 1, "point_weights") != n:
        raise ValueError(f"point_weights holds {_n_rows(point_weights, 1, 'point_weights')} values for {n} points")
    if m == 0:
        z = np.zeros(0, np.float64)
        diag = {k: z.copy() for k in _EV_NAMES if k not in ("Lambda_ell", "theta_ell")}
        diag["n_in_radius"] = np.zeros(0, np.int32)
        return (z, z.copy(), diag) if return_diag else (z, z.copy())
    ctx = ctx or _abi.default_context()
    dp = _abi.device_input(ctx, points_camera_frame, np.float64, (n, 3)) if n else None
    dw = _abi.device_input(ctx, point_weights, np.float64, (n,)) if (point_weights is not None and n) else None
    (duv,) = _abi.upload_many(ctx, [uv.reshape(m, 2)])
    d_ev, d_cnt = _abi.alloc_many(ctx, [((m, _abi.GC_CAM_EV), np.float64), ((m,), np.int32)])
    _abi.call("gc_lidar_depth_evidence", ctx.handle, n, dp.ptr if dp else None, m, duv.ptr, h_k.ctypes.data,
              C.byref(c_cfg), dw.ptr if dw else None, d_ev.ptr, d_cnt.ptr, ctx=ctx)
    ev, cnt = _abi.download_many([d_ev, d_cnt])
    out = {k: np.ascontiguousarray(ev[:, q]) for q, k in enumerate(_EV_NAMES)}
    if not return_diag:
        return out["Lambda_ell"], out["theta_ell"]
    diag = {k: out[k] for k in _EV_NAMES if k not in ("Lambda_ell", "theta_ell")}
    diag["n_in_radius"] = cnt.copy()
    return out["Lambda_ell"], out["theta_ell"], diag


def _batch_block(ctx, n_total: int, n_lobes: int, extra=()):
    names = list(BATCH_ARRAYS)
    shapes = {k: (n_total,) + (shp if k != "etas" else (n_lobes, 3)) for k, (shp, _, _) in BATCH_ARRAYS.items()}
    blk = _abi.alloc_many(ctx, [(shapes[k], BATCH_ARRAYS[k][2]) for k in names] + list(extra))
    return names, blk


def _finish_batch(names, blk, counts, device_out: bool):
    out = dict(zip(names, blk[:len(names)]))
    if device_out:
        return MeasurementBatch(**out, **counts, device=dict(out)), None
    host = _abi.download_many(blk)
    arrays = {k: v.astype(BATCH_ARRAYS[k][1], copy=False) for k, v in zip(names, host)}
    return MeasurementBatch(**arrays, **counts), host[len(names):]


def measurement_batch_from_camera_splats(positions, covariances, directions, kappas, weights, timestamps,
                                         colors=None, n_feat: int = GC_N_FEAT, n_surfel: int = GC_N_SURFEL,
                                         eps_lift: float = GC_EPS_LIFT, *, ctx=None,
                                         device_out: bool = False) -> MeasurementBatch:
    """measurement_batch.py:165-259: rows [0, min(N, n_feat)) in information form with one vMF lobe;
    the rest of the batch zero. Inputs may be DeviceArrays."""
    _check_budget(n_feat, n_surfel)
    n = _n_rows(positions, 3, "positions")
    if n > 1 << 24:
        raise ValueError(f"{n} splats; at most 2^24 are supported")
    wants = (("covariances", covariances, 9), ("directions", directions, 3), ("kappas", kappas, 1),
             ("weights", weights, 1), ("timestamps", timestamps, 1)) + ((("colors", colors, 3),) if colors is not None
                                                                       else ())
    for what, x, width in wants:
        got = _n_rows(x, width, what)
        if got != n:
            raise ValueError(f"{what} holds {got} rows for {n} positions")
    if not math.isfinite(float(eps_lift)):
        raise ValueError(f"eps_lift must be finite, got {eps_lift}")
    n_feat, n_surfel = int(n_feat), int(n_surfel)
    counts = dict(n_feat=n_feat, n_surfel=n_surfel, n_camera_valid=min(n, n_feat), n_lidar_valid=0)
    ctx = ctx or _abi.default_context()
    names, blk = _batch_block(ctx, n_feat + n_surfel, GC_VMF_N_LOBES)
    ins = [None] * 7
    if n:
        arrs = [positions, covariances, directions, kappas, weights, timestamps] + ([colors] if colors is not None else [])
        shp = [(n, 3), (n, 3, 3), (n, 3), (n,), (n,), (n,), (n, 3)]
        arrs = [a if isinstance(a, _abi.DeviceArray) else _host_rows(a, s, "a splat array") for a, s in zip(arrs, shp)]
        dev = _abi.upload_many(ctx, arrs)
        ins[:len(dev)] = [_abi.device_input(ctx, d, np.float64, s).ptr for d, s in zip(dev, shp)]
    _abi.call("gc_measurement_batch_from_camera_splats", ctx.handle, n, *ins, n_feat, n_surfel, GC_VMF_N_LOBES,
              float(eps_lift), *[b.ptr for b in blk], ctx=ctx)
    return _finish_batch(names, blk, counts, device_out)[0]


def feature_list_to_camera_batch(features: Sequence, timestamp_sec: float, n_feat: int = GC_N_FEAT,
                                 n_surfel: int = GC_N_SURFEL, eps_lift: float = GC_EPS_LIFT, *, ctx=None,
                                 device_out: bool = False) -> MeasurementBatch:
    """camera_batch_utils.py:23-86. features: objects with the Feature3D attributes xyz, cov_xyz,
    weight, kappa_app, mu_app (or None) and optionally color (duck-typed). The packing (truncation
    to n_feat, the direction mu_app or xyz over its norm + 1e-12, grey 0.5 without a colour, one
    timestamp) is the reference's host code; the batch rows are computed on the device."""
    _check_budget(n_feat, n_surfel)
    if not features:
        return create_empty_measurement_batch(n_feat=n_feat, n_surfel=n_surfel)
    fs = list(features)[:min(len(features), int(n_feat))]
    n = len(fs)
    positions = np.array([np.asarray(f.xyz, np.float64).reshape(3) for f in fs], np.float64).reshape(n, 3)
    covariances = np.array([np.asarray(f.cov_xyz, np.float64).reshape(3, 3) for f in fs], np.float64).reshape(n, 3, 3)
    weights = np.array([f.weight for f in fs], np.float64)
    kappas = np.array([f.kappa_app for f in fs], np.float64)
    timestamps = np.full(n, timestamp_sec, np.float64)
    colors = np.full((n, 3), 0.5, np.float64)
    directions = np.zeros((n, 3), np.float64)
    for i, f in enumerate(fs):
        c = getattr(f, "color", None)
        if c is not None and np.size(c) >= 3:
            colors[i] = np.asarray(c, np.float64).ravel()[:3]
        d = np.asarray(f.mu_app if getattr(f, "mu_app", None) is not None else f.xyz, np.float64).reshape(3)
        directions[i] = d / (np.linalg.norm(d) + 1e-12)
    return measurement_batch_from_camera_splats(positions, covariances, directions, kappas, weights, timestamps,
                                                colors, n_feat=n_feat, n_surfel=n_surfel, eps_lift=eps_lift,
                                                ctx=ctx, device_out=device_out)


_FEATURE_SHAPES = (("u", ()), ("v", ()), ("depth_Lambda_c", ()), ("depth_theta_c", ()), ("weight", ()),
                   ("kappa_app", ()), ("mu_app", (3,)), ("has_mu_app", ()), ("color", (3,)), ("has_color", ()),
                   ("xyz", (3,)), ("cov_xyz", (3, 3)))


def _pack_features(features: CameraFeatures):
    m = len(features)
    out = {}
    for name, shp in _FEATURE_SHAPES:
        x = getattr(features, name)
        if name.startswith("has_"):
            a = np.ascontiguousarray(np.asarray(x).astype(bool).astype(np.uint8))
            if a.shape != (m,):
                raise ValueError(f"features.{name} of shape {a.shape}, expected ({m},)")
        else:
            a = _host_rows(x, (m,) + shp, f"features.{name}") if np.size(x) == m * int(np.prod(shp, dtype=int)) else None
            if a is None:
                raise ValueError(f"features.{name} of shape {np.shape(x)}, expected {(m,) + shp}")
        out[name] = a
    return out


def camera_measurement_batch(points_base, features, intrinsics: PinholeIntrinsics, R_base_camera,
                             t_base_camera, timestamp_sec: float,
                             config: Optional[LidarCameraDepthFusionConfig] = None, *, pixel_sigma: float = 1.0,
                             n_feat: int = GC_N_FEAT, n_surfel: int = GC_N_SURFEL, eps_lift: float = GC_EPS_LIFT,
                             ctx=None, device_out: bool = False, return_diag: bool = False):
    """backend_node.py:1872-1925 in one device call: base-frame LiDAR points (N, 3; host array or the
    DeviceArray deskew_constant_twist(..., device_out=True) returns) and the image's features (a host
    CameraFeatures, or the DeviceCameraFeatures lift_camera_features(..., device_out=True) returns,
    whose arrays are read where they lie) -> the camera slice of a fresh MeasurementBatch in the base
    frame (rows past min(M, n_feat) zero), which extract_lidar_surfels takes as base_batch. With device_out the nine arrays stay in HBM as the
    batch's fields and batch.device. With return_diag the result is (batch, CameraSplatDiagnostics).
    No features gives create_empty_measurement_batch, as feature_list_to_camera_batch does."""
    cfg = config or LidarCameraDepthFusionConfig()
    c_cfg = _cfg(cfg)
    h_k = _intr_vector(intrinsics.fx, intrinsics.fy, intrinsics.cx, intrinsics.cy)
    _check_budget(n_feat, n_surfel)
    n_feat, n_surfel = int(n_feat), int(n_surfel)
    R = _host_rows(R_base_camera, (3, 3), "R_base_camera")
    t = _host_rows(t_base_camera, (3,), "t_base_camera")
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        raise ValueError("R_base_camera and t_base_camera must be finite")
    scal = dict(pixel_sigma=pixel_sigma, timestamp_sec=timestamp_sec, eps_lift=eps_lift)
    for k, v in scal.items():
        if math.isnan(float(v)):
            raise ValueError(f"{k} is NaN")
    n = _n_rows(points_base, 3, "points_base")
    m = len(features)
    _check_counts(n, m)
    on_device = isinstance(features, DeviceCameraFeatures)
    f = None if on_device else _pack_features(features)
    if m == 0:
        empty = create_empty_measurement_batch(n_feat=n_feat, n_surfel=n_surfel)
        return (empty, None) if return_diag else empty
    ctx = ctx or (features.uv.ctx if on_device else _abi.default_context())
    dp = _abi.device_input(ctx, points_base, np.float64, (n, 3)) if n else None
    if on_device:  # the lift's arrays where they lie in HBM: no download, no upload
        dev = [_abi.device_input(ctx, getattr(features, k), np.uint8 if k.startswith("has_") else np.float64,
                                 (m,) + shp) for k, shp in (("uv", (2,)),) + _FEATURE_SHAPES[2:]]
    else:
        uv = np.stack([f["u"], f["v"]], axis=1)
        order = [uv, f["depth_Lambda_c"], f["depth_theta_c"], f["weight"], f["kappa_app"], f["mu_app"],
                 f["has_mu_app"], f["color"], f["has_color"], f["xyz"], f["cov_xyz"]]
        dts = [np.uint8 if a.dtype == np.uint8 else np.float64 for a in order]
        dev = _abi.upload_many(ctx, order, dts)
    extra = [((m, 3), np.float64), ((m, 3, 3), np.float64), ((m,), np.uint8), ((m, _abi.GC_CAM_EV), np.float64),
             ((m,), np.int32)]
    names, blk = _batch_block(ctx, n_feat + n_surfel, GC_VMF_N_LOBES, extra)
    _abi.call("gc_camera_measurement_batch", ctx.handle, n, dp.ptr if dp else None, R.ctypes.data, t.ctypes.data, m,
              *[d.ptr for d in dev], h_k.ctypes.data, C.byref(c_cfg), float(pixel_sigma), float(timestamp_sec),
              n_feat, n_surfel, GC_VMF_N_LOBES, float(eps_lift), *[b.ptr for b in blk], ctx=ctx)
    counts = dict(n_feat=n_feat, n_surfel=n_surfel, n_camera_valid=min(m, n_feat), n_lidar_valid=0)
    batch, rest = _finish_batch(names, blk, counts, device_out)
    if not return_diag:
        return batch
    if rest is None:
        rest = _abi.download_many(blk)[len(names):]
    fxyz, fcov, fflag, ev, cnt = rest
    diag = CameraSplatDiagnostics(xyz=fxyz.copy(), cov_xyz=fcov.copy(), fused=fflag.astype(bool), n_in_radius=cnt.copy(),
                                  **{k: np.ascontiguousarray(ev[:, q]) for q, k in enumerate(_EV_NAMES)})
    return batch, diag
