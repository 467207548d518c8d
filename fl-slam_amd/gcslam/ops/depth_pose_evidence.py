"""Depth pose evidence from the camera view ("Depth pose evidence"): Gaussian pose evidence
(L, h) of an observed depth frame against the depth image the camera view renders from the device map,
in visual_pose_evidence's coordinates, so that it adds to that operator's evidence and goes through
set_lidar_evidence with it. The operator is this build's: the reference has no renderer in its estimator.

The pose derivative of every pixel's rendered depth is carried forward through the compositing loop as
six tangents (csrc/gc_depthev.hip); there is no backward pass. The tangent convention is
visual_pose_evidence.py's (r = map - (R m + t) with d/dt = -I, :89-99; R_delta = R_scatter R_pred^T,
:234-238): delta = [dt, dtheta] with t_wb' = t_wb + dt and R_wb' = Exp(dtheta) R_wb.

The host side is the one driver of the camera view's evidences (camview_pose_evidence.py): four device calls
(gc_camera_splat_prep, gc_camera_splat_jvp, gc_render_depth_tiles, gc_depth_pose_evidence) with no wait
between them; every argument error is raised there before a device is asked for."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from ..certificates import CertBundle, ExpectedEffect
from ..constants import GC_CHART_ID, GC_EPS_LIFT
from . import camview_pose_evidence as camview
from .camera_features import DEPTH_MODELS, VisualFeatureConfig
from .camview_pose_evidence import MAX_POSES, MAX_TILE  # noqa: F401  (their import path of old)


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

    def check(self):
        if self.depth_model not in DEPTH_MODELS:
            raise ValueError(f"Unknown depth_model: {self.depth_model!r}; one of {DEPTH_MODELS}")
        vals = [self.depth_sigma0, self.depth_sigma_slope, self.min_depth_m, self.max_depth_m, self.eps_lift]
        if self.robust_nu is not None:
            vals.append(self.robust_nu)
        if not np.isfinite(np.asarray(vals, np.float64)).all():
            raise ValueError("the depth evidence configuration must be finite")
        if not (self.depth_sigma0 > 0.0 and self.depth_sigma_slope >= 0.0):
            raise ValueError(f"depth_sigma0 must be > 0 and depth_sigma_slope >= 0, got {self.depth_sigma0}, "
                             f"{self.depth_sigma_slope}")
        if not 0.0 <= self.min_depth_m < self.max_depth_m:
            raise ValueError(f"the depth limits must satisfy 0 <= min_depth_m < max_depth_m, got {self.min_depth_m}, "
                             f"{self.max_depth_m}")
        if self.robust_nu is not None and not self.robust_nu > 0.0:
            raise ValueError(f"robust_nu must be > 0 or None, got {self.robust_nu}")
        if self.eps_lift < 0.0:
            raise ValueError(f"eps_lift must be >= 0, got {self.eps_lift}")


class DepthPoseEvidenceResult(camview.PoseEvidenceResult):
    """The depth evidence's result: PoseEvidenceResult's fields."""


result_from_parts = camview.parts_row_reader(DepthPoseEvidenceResult, "depth_pose_evidence", "render_depth_residual")


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
    view = camview.prepare(batch_or_map, intrinsics, poses6, (depth_obs, cfg or DepthEvidenceConfig()), None, R_base_camera,
                           t_base_camera, view_cfg, accumulate_into)
    return camview.evidence(view, device_out, return_images)


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
    return result_from_parts(Lp[0], hp[0], parts[0], render["depth"].shape[1:], cfg.eps_lift, chart_id, anchor_id)
