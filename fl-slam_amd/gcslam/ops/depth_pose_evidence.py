"""Depth pose evidence from the camera view ("Depth pose evidence"): Gaussian pose evidence
(L, h) of an observed depth frame against the depth image the camera view renders from the device map,
in visual_pose_evidence's coordinates, so that it adds to that operator's evidence and goes through
set_lidar_evidence with it. The operator is this build's: the reference has no renderer in its estimator.

The pose derivative of every pixel's rendered depth is carried forward through the compositing loop as
six tangents (csrc/gc_depthev.hip); there is no backward pass. The tangent convention is
visual_pose_evidence.py's (r = map - (R m + t) with d/dt = -I, :89-99; R_delta = R_scatter R_pred^T,
:234-238): delta = [dt, dtheta] with t_wb' = t_wb + dt and R_wb' = Exp(dtheta) R_wb.

Four device calls (gc_camera_splat_prep, gc_camera_splat_jvp, gc_render_depth_tiles,
gc_depth_pose_evidence) with no wait between them; every argument error is raised here before a device
is asked for."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np

from .. import _abi, rendering
from ..certificates import CertBundle, ExpectedEffect, InfluenceCert, SupportCert
from ..constants import D_Z, GC_CHART_ID, GC_EPS_LIFT
from .camera_features import DEPTH_MODELS, VisualFeatureConfig, _depth_image
from .camera_splats import PinholeIntrinsics

MAX_POSES = _abi.GC_RENDER_MAX_VIEWS
MAX_TILE = 16  # a thread owns one pixel


@dataclass(frozen=True)
class DepthEvidenceConfig:
    """sigma(d) is the camera features' depth model (VisualFeatureConfig: sigma0 + slope d, or
    sigma0 + slope d^2), the depth limits default to that configuration's; robust_nu is the Student-t
    degrees of freedom of the IRLS weight (nu + 1) / (nu + (r / sigma)^2), None for none."""
    depth_model: str = "linear"
    depth_sigma0: float = 0.01
    depth_sigma_slope: float = 0.01
    min_depth_m: float = VisualFeatureConfig.min_depth_m
    max_depth_m: float = VisualFeatureConfig.max_depth_m
    robust_nu: Optional[float] = None
    eps_lift: float = GC_EPS_LIFT


@dataclass
class DepthPoseEvidenceResult:
    L_pose: np.ndarray  # (22, 22)
    h_pose: np.ndarray  # (22,)
    L6: np.ndarray      # (6, 6) sum w J J^T, without the lift
    h6: np.ndarray      # (6,)
    total_weighted_cost: float
    n_used: int
    sum_coverage: float
    sum_weight: float


def _check_cfg(cfg: DepthEvidenceConfig):
    if cfg.depth_model not in DEPTH_MODELS:
        raise ValueError(f"Unknown depth_model: {cfg.depth_model!r}; one of {DEPTH_MODELS}")
    vals = [cfg.depth_sigma0, cfg.depth_sigma_slope, cfg.min_depth_m, cfg.max_depth_m, cfg.eps_lift]
    if cfg.robust_nu is not None:
        vals.append(cfg.robust_nu)
    if not np.isfinite(np.asarray(vals, np.float64)).all():
        raise ValueError("the depth evidence configuration must be finite")
    if not (cfg.depth_sigma0 > 0.0 and cfg.depth_sigma_slope >= 0.0):
        raise ValueError(f"depth_sigma0 must be > 0 and depth_sigma_slope >= 0, got {cfg.depth_sigma0}, "
                         f"{cfg.depth_sigma_slope}")
    if not 0.0 <= cfg.min_depth_m < cfg.max_depth_m:
        raise ValueError(f"the depth limits must satisfy 0 <= min_depth_m < max_depth_m, got {cfg.min_depth_m}, "
                         f"{cfg.max_depth_m}")
    if cfg.robust_nu is not None and not cfg.robust_nu > 0.0:
        raise ValueError(f"robust_nu must be > 0 or None, got {cfg.robust_nu}")
    if cfg.eps_lift < 0.0:
        raise ValueError(f"eps_lift must be >= 0, got {cfg.eps_lift}")


def _check_frame(intrinsics, poses6, R_base_camera, t_base_camera, view_cfg, what: str = "the depth evidence"):
    """What the evidences of the camera view refuse of the poses, the extrinsics and the tiles without a
    device: (P, host poses or None, Rbc, tbc)."""
    if not isinstance(intrinsics, PinholeIntrinsics):
        raise ValueError("intrinsics must be a PinholeIntrinsics")
    if int(view_cfg.tile_size) != view_cfg.tile_size or not 1 <= view_cfg.tile_size <= MAX_TILE:
        raise ValueError(f"tile_size must be an integer in [1, {MAX_TILE}] for {what} (a thread owns one "
                         f"pixel), got {view_cfg.tile_size}")
    if isinstance(poses6, _abi.DeviceArray):
        if poses6.dtype != np.float64 or int(np.prod(poses6.shape)) % 6:
            raise ValueError(f"device poses6 of dtype {poses6.dtype} and shape {poses6.shape}, expected float64 (P, 6)")
        P, host = int(np.prod(poses6.shape)) // 6, None
    else:
        host = np.ascontiguousarray(poses6, np.float64)
        if host.ndim == 1 and host.size == 6:
            host = host.reshape(1, 6)
        if host.ndim != 2 or host.shape[1] != 6:
            raise ValueError(f"poses6 of shape {host.shape}, expected (P, 6)")
        P = host.shape[0]
        if not np.isfinite(host).all():
            raise ValueError("poses6 must be finite")
    if not 1 <= P <= MAX_POSES:
        raise ValueError(f"{P} poses; between 1 and {MAX_POSES} are supported")
    Rbc, tbc = rendering._extrinsics(R_base_camera, t_base_camera)
    if not (np.isfinite(Rbc).all() and np.isfinite(tbc).all()):
        raise ValueError("the extrinsics must be finite")
    if np.max(np.abs(Rbc.T @ Rbc - np.eye(3))) > 1e-9:
        raise ValueError("R_base_camera must be a rotation (max |R^T R - I| <= 1e-9)")
    return P, host, Rbc, tbc


def _check_accumulate(accumulate_into, P: int):
    if accumulate_into is not None:
        try:
            dL, dh = accumulate_into
        except (TypeError, ValueError):
            raise ValueError("accumulate_into must be (L_pose, h_pose)") from None
        for a, sh in ((dL, (P, D_Z, D_Z)), (dh, (P, D_Z))):
            if not isinstance(a, _abi.DeviceArray) or a.dtype != np.float64 or int(np.prod(a.shape)) != int(np.prod(sh)):
                raise ValueError(f"accumulate_into holds float64 DeviceArrays of {P} x 22 x 22 and {P} x 22 values")


def _check_args(intrinsics, poses6, depth_obs, R_base_camera, t_base_camera, view_cfg, cfg, accumulate_into):
    """Everything that can be refused without a device: (P, host poses or None, Rbc, tbc, H, W, depth_obs as
    the device reads it)."""
    if not isinstance(intrinsics, PinholeIntrinsics):
        raise ValueError("intrinsics must be a PinholeIntrinsics")
    _check_cfg(cfg)
    P, host, Rbc, tbc = _check_frame(intrinsics, poses6, R_base_camera, t_base_camera, view_cfg)
    H, W, depth_obs = _depth_image(depth_obs, "depth_obs")
    rendering._check_camera_args(intrinsics, np.eye(4), H, W, view_cfg, 0)
    _check_accumulate(accumulate_into, P)
    return P, host, Rbc, tbc, H, W, depth_obs


def depth_pose_evidence_batched(batch_or_map, intrinsics, poses6, depth_obs, R_base_camera=None, t_base_camera=None,
                                view_cfg=None, cfg: Optional[DepthEvidenceConfig] = None, accumulate_into=None,
                                device_out: bool = False, return_images: bool = False):
    """The depth evidence of P linearisation body poses poses6 (P, 6) = [t, rotvec] (1 <= P <= 32; a host
    array or a DeviceArray, as visual_pose_evidence_batched takes) from one observed depth image
    depth_obs (H, W; metres, float32; host or DeviceArray, lift_camera_features' conventions) and a
    renderable batch (or a DevicePrimitiveMap: publish_renderable first), seen through `intrinsics` at
    the extrinsics R_base_camera, t_base_camera (default: the camera at the body).

    Returns (L_pose (P, 22, 22), h_pose (P, 22), parts (P, GC_DEPTHEV_PARTS), render): parts rows are
    [L6 (36) | h6 (6) | cost | n_used | sum_cov | sum_w]; render is the dict of DeviceArrays of the four
    calls (depth, alpha, n_contrib, the tile lists, the splats and their tangents dmeans_px, ddepths,
    dSigmas_inv; with return_images also residual and weight (P, H, W)). Row p is bitwise the single
    call for pose p. accumulate_into = (L_pose, h_pose) DeviceArrays: L6 and h6 are added into them on
    the device (no lift) and they are what comes back. With device_out L_pose and h_pose stay
    DeviceArrays. The four device calls run with no wait between them; device poses are read once
    before the first."""
    view_cfg = view_cfg or rendering.CameraViewConfig()
    cfg = cfg or DepthEvidenceConfig()
    P, host, Rbc, tbc, H, W, depth_obs = _check_args(intrinsics, poses6, depth_obs, R_base_camera, t_base_camera,
                                                     view_cfg, cfg, accumulate_into)
    batch = rendering._device_batch(batch_or_map, None)
    ctx, n = batch.ctx, batch.count
    if host is None:
        host = poses6.download().reshape(P, 6)
        if not np.isfinite(host).all():
            raise ValueError("poses6 must be finite")
    T_cw = rendering.camera_from_world(host, Rbc, tbc, ctx=ctx)
    t_wb = np.ascontiguousarray(host[:, :3])
    Ks = [intrinsics] * P
    c_cfg, T_cw, K = rendering._check_camera_args(Ks, T_cw, H, W, view_cfg, n)
    ts, cap = int(view_cfg.tile_size), int(view_cfg.max_splats_per_tile)
    d_obs = depth_obs if isinstance(depth_obs, _abi.DeviceArray) else _abi.DeviceArray.from_host(ctx, depth_obs, np.float32)

    splats = rendering.camera_splat_prep(batch, Ks, T_cw, H, W, view_cfg)
    st = rendering._CamSplatStruct(*[splats[k].ptr for k, _ in rendering._CamSplatStruct._fields_])
    dm, dz, dS = _abi.alloc_many(ctx, [(P, n, 6, 2), (P, n, 6), (P, n, 6, 3)])
    _abi.call("gc_camera_splat_jvp", ctx.handle, C.byref(batch.struct), n, P, T_cw.ctypes.data, t_wb.ctypes.data,
              K.ctypes.data, H, W, C.byref(c_cfg), C.byref(st), dm.ptr, dz.ptr, dS.ptr, ctx=ctx)
    dev = rendering.render_depth_tiles(splats, H, W, view_cfg, ctx=ctx)
    if accumulate_into is not None:
        dL = _abi.device_input(ctx, accumulate_into[0], np.float64, (P, D_Z, D_Z))
        dh = _abi.device_input(ctx, accumulate_into[1], np.float64, (P, D_Z))
        (dparts,) = _abi.alloc_many(ctx, [(P, _abi.GC_DEPTHEV_PARTS)])
    else:
        dL, dh, dparts = _abi.alloc_many(ctx, [(P, D_Z, D_Z), (P, D_Z), (P, _abi.GC_DEPTHEV_PARTS)])
    d_res = d_w = None
    if return_images:
        d_res, d_w = _abi.alloc_many(ctx, [(P, H, W), (P, H, W)])
    _abi.call("gc_depth_pose_evidence", ctx.handle, P, n, C.byref(st), dm.ptr, dz.ptr, dS.ptr, H, W, ts, cap,
              C.byref(c_cfg), dev["tile_counts"].ptr, dev["tile_indices"].ptr, dev["alpha"].ptr, dev["depth"].ptr,
              d_obs.ptr, DEPTH_MODELS.index(cfg.depth_model), float(cfg.depth_sigma0), float(cfg.depth_sigma_slope),
              float(cfg.min_depth_m), float(cfg.max_depth_m), int(cfg.robust_nu is not None),
              float(cfg.robust_nu or 0.0), float(cfg.eps_lift), int(accumulate_into is not None), dL.ptr, dh.ptr,
              dparts.ptr, d_res.ptr if d_res is not None else None, d_w.ptr if d_w is not None else None, ctx=ctx)
    render: Dict[str, _abi.DeviceArray] = dict(dev, **splats, dmeans_px=dm, ddepths=dz, dSigmas_inv=dS, depth_obs=d_obs)
    if return_images:
        render.update(residual=d_res, weight=d_w)
    if device_out:
        return dL, dh, dparts.download(), render
    if accumulate_into is None:
        Lp, hp, parts = _abi.download_many([dL, dh, dparts])
        return Lp.copy(), hp.copy(), parts.copy(), render
    return dL.download(), dh.download(), dparts.download(), render


def depth_pose_evidence(batch_or_map, intrinsics, pose6, depth_obs, R_base_camera=None, t_base_camera=None,
                        view_cfg=None, cfg: Optional[DepthEvidenceConfig] = None, chart_id: str = GC_CHART_ID,
                        anchor_id: str = "depth_pose_evidence"
                        ) -> Tuple[DepthPoseEvidenceResult, CertBundle, ExpectedEffect]:
    """The operator for one linearisation pose [t, rotvec]: (DepthPoseEvidenceResult, CertBundle,
    ExpectedEffect). The certificate is approximate (triggers linearization and render_depth_residual,
    support = (sum of the used pixels' coverage, n_used / (H W)), lift_strength = eps_lift), and exact
    when no pixel is used (L6 = 0, h = 0)."""
    cfg = cfg or DepthEvidenceConfig()
    pose = np.asarray(pose6, np.float64).ravel()[:6]
    Lp, hp, parts, render = depth_pose_evidence_batched(batch_or_map, intrinsics, pose[None], depth_obs, R_base_camera,
                                                        t_base_camera, view_cfg, cfg)
    result, cert, effect = result_from_parts(Lp[0], hp[0], parts[0], render["depth"].shape[1:], cfg.eps_lift, chart_id,
                                             anchor_id)
    return result, cert, effect


def result_from_parts(L_pose, h_pose, parts, image_shape, eps_lift: float = GC_EPS_LIFT, chart_id: str = GC_CHART_ID,
                      anchor_id: str = "depth_pose_evidence"):
    """One parts row as (DepthPoseEvidenceResult, CertBundle, ExpectedEffect)."""
    p = np.asarray(parts, np.float64)
    cost, n_used, sum_cov, sum_w = float(p[42]), int(p[43]), float(p[44]), float(p[45])
    result = DepthPoseEvidenceResult(L_pose=L_pose, h_pose=h_pose, L6=p[0:36].reshape(6, 6).copy(), h6=p[36:42].copy(),
                                     total_weighted_cost=cost, n_used=n_used, sum_coverage=sum_cov, sum_weight=sum_w)
    if n_used == 0:
        return (result, CertBundle.create_exact(chart_id=chart_id, anchor_id=anchor_id),
                ExpectedEffect(objective_name="depth_pose_evidence", predicted=0.0, realized=0.0))
    H, W = image_shape
    cert = CertBundle.create_approx(
        chart_id=chart_id, anchor_id=anchor_id, triggers=["linearization", "render_depth_residual"],
        frobenius_applied=False, support=SupportCert(ess_total=sum_cov, support_frac=n_used / float(H * W)),
        influence=InfluenceCert.identity().with_overrides(lift_strength=eps_lift))
    return result, cert, ExpectedEffect(objective_name="depth_pose_evidence", predicted=cost, realized=cost)
