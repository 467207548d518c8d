"""Photometric pose evidence from the camera view ("Photometric pose evidence"): Gaussian pose
evidence (L, h) of an observed image against the colour the camera view renders from the device map, one
luminance channel y = (w_r r + w_g g) + w_b b, in depth_pose_evidence's coordinates and conventions, so that
the two add; rgbd_pose_evidence_batched gives both from one prep, one set of tile lists and one forward
raster. The operator is this build's: the reference has no renderer in its estimator.

The residual is r = Y / A - lum_obs, the rendered luminance over the coverage (as the rendered depth is
D / A), so it does not read the background colour: a pixel at the frontier of an incomplete map is held
against what the map shows there. The pose derivative carries the tangent of the vMF shading towards the
camera (gc_camera_shade_jvp) and the six tangents of every pixel's (T, Y) forward through the compositing
loop (csrc/gc_depthev.hip); there is no backward pass. delta = [dt, dtheta] with t_wb' = t_wb + dt and
R_wb' = Exp(dtheta) R_wb.

The host side is the one driver of the camera view's evidences (camview_pose_evidence.py): every argument
error is raised there before a device is asked for; the device calls run with no wait between them."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .. import _abi
from ..certificates import CertBundle, ExpectedEffect
from ..constants import GC_CHART_ID, GC_EPS_LIFT
from . import camview_pose_evidence as camview
from .depth_pose_evidence import DepthEvidenceConfig

GREY_WEIGHTS = (4899.0 / 16384.0, 9617.0 / 16384.0, 1868.0 / 16384.0)  # the keypoint detector's grey

# Whether rgbd_pose_evidence_batched makes the one joint call (gc_rgbd_pose_evidence) or the depth call and
# then the luminance call, when the caller does not say: the bytes are the same either way, the choice is
# the measured one. The joint entry's median is below the two single entries' sum by more than the two
# p10-p90 spreads together in all four shapes of tools/probe/time_photo_evidence.py (DESIGN.md §4,
# "Photometric pose evidence", measured times).
RGBD_JOINT_DEFAULT = True


def _weights(weights) -> np.ndarray:
    try:
        w = np.ascontiguousarray(GREY_WEIGHTS if weights is None else weights, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"weights must hold 3 finite values, got {weights!r}") from None
    if w.shape != (3,) or not np.isfinite(w).all():
        raise ValueError(f"weights must hold 3 finite values, got {weights!r}")
    return w


@dataclass(frozen=True)
class PhotometricEvidenceConfig:
    """sigma is the standard deviation of a luminance residual; 0.05 is this build's choice for a luminance
    in [0, 1] (5 % of the range: sensor noise plus what the map's one colour per primitive cannot say), not
    the reference's. weights is the luminance triple (any finite values; the default is the keypoint
    detector's grey). robust_nu is the Student-t degrees of freedom of the IRLS weight
    (nu + 1) / (nu + (r / sigma)^2), None for none."""
    sigma: float = 0.05
    weights: Tuple[float, float, float] = GREY_WEIGHTS
    robust_nu: Optional[float] = None
    eps_lift: float = GC_EPS_LIFT

    def check(self) -> np.ndarray:
        """The luminance weights as the device reads them."""
        w = _weights(self.weights)
        vals = [self.sigma, self.eps_lift] + ([] if self.robust_nu is None else [self.robust_nu])
        if not np.isfinite(np.asarray(vals, np.float64)).all():
            raise ValueError("the photometric evidence configuration must be finite")
        if not self.sigma > 0.0:
            raise ValueError(f"sigma must be > 0, got {self.sigma}")
        if self.robust_nu is not None and not self.robust_nu > 0.0:
            raise ValueError(f"robust_nu must be > 0 or None, got {self.robust_nu}")
        if self.eps_lift < 0.0:
            raise ValueError(f"eps_lift must be >= 0, got {self.eps_lift}")
        return w


class PhotometricPoseEvidenceResult(camview.PoseEvidenceResult):
    """The photometric evidence's result: PoseEvidenceResult's fields."""


result_from_parts = camview.parts_row_reader(PhotometricPoseEvidenceResult, "photometric_pose_evidence",
                                             "render_photometric_residual")


def luminance_image(rgb, weights=None, *, ctx=None, device_out: bool = False):
    """An (H, W, 3) uint8 rgb image (host or DeviceArray) as the float32 luminance
    ((w_r R + w_g G) + w_b B) / 255, summed in f64 (gc_image_luminance): what the evidence observes."""
    w = _weights(weights)
    H, W, is_rgb, img = camview.image_obs(rgb, "rgb")
    if not is_rgb:
        raise ValueError(f"rgb of shape {(H, W)}, expected (H, W, 3)")
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise ValueError(f"H and W must be in [1, 16384], got {H}, {W}")
    ctx = ctx or (img.ctx if isinstance(img, _abi.DeviceArray) else _abi.default_context())
    d = camview.luminance_device(ctx, img, H, W, w)
    return d if device_out else d.download()


def photometric_pose_evidence_batched(batch_or_map, intrinsics, poses6, image_obs, R_base_camera=None, t_base_camera=None,
                                      view_cfg=None, cfg: Optional[PhotometricEvidenceConfig] = None, accumulate_into=None,
                                      device_out: bool = False, return_images: bool = False):
    """The photometric evidence of P linearisation body poses poses6 (P, 6) = [t, rotvec] (1 <= P <= 32; a
    host array or a DeviceArray) from one observed image image_obs, (H, W, 3) uint8 rgb or an (H, W) float
    luminance in which NaN marks a hole (host or DeviceArray), and a renderable batch (or a
    DevicePrimitiveMap: publish_renderable first), with depth_pose_evidence_batched's arguments and
    conventions.

    Returns (L_pose (P, 22, 22), h_pose (P, 22), parts (P, GC_DEPTHEV_PARTS), render): parts rows are
    [L6 (36) | h6 (6) | cost | n_used | sum_cov | sum_w]; render is the dict of DeviceArrays of the calls
    (alpha, n_contrib, the tile lists, the splats, their tangents, lum (P, n), dlum (P, n, 6), lum_obs;
    with return_images also lum_render = Y / A, residual and weight (P, H, W)). Row p is bitwise the
    single call for pose p. accumulate_into and device_out as in depth_pose_evidence_batched. No wait
    between the device calls."""
    if image_obs is None:
        raise ValueError("image_obs is None")
    view = camview.prepare(batch_or_map, intrinsics, poses6, None, (image_obs, cfg or PhotometricEvidenceConfig()),
                           R_base_camera, t_base_camera, view_cfg, accumulate_into)
    return camview.evidence(view, device_out, return_images)


def rgbd_pose_evidence_batched(batch_or_map, intrinsics, poses6, depth_obs, image_obs, R_base_camera=None,
                               t_base_camera=None, view_cfg=None, depth_cfg: Optional[DepthEvidenceConfig] = None,
                               photo_cfg: Optional[PhotometricEvidenceConfig] = None, accumulate_into=None,
                               device_out: bool = False, return_images: bool = False, joint: Optional[bool] = None):
    """Both evidences of an RGB-D frame, summed: the depth's L6 and h6 and then the luminance's (one lift,
    so depth_cfg.eps_lift and photo_cfg.eps_lift must agree), from one prep, one set of tile lists and one
    forward raster. parts is (P, 2, GC_DEPTHEV_PARTS), the depth row first, each row the bytes of its own
    operator; with return_images render holds residual, weight (the depth's), lum_render, lum_residual and
    lum_weight. joint: True for the one-pass entry gc_rgbd_pose_evidence, False for the depth entry followed
    by the luminance entry, None for the measured default (RGBD_JOINT_DEFAULT); the bytes are the same."""
    if depth_obs is None or image_obs is None:
        raise ValueError("depth_obs and image_obs are both needed")
    view = camview.prepare(batch_or_map, intrinsics, poses6, (depth_obs, depth_cfg or DepthEvidenceConfig()),
                           (image_obs, photo_cfg or PhotometricEvidenceConfig()), R_base_camera, t_base_camera, view_cfg,
                           accumulate_into)
    return camview.evidence(view, device_out, return_images, RGBD_JOINT_DEFAULT if joint is None else joint)


def photometric_pose_evidence(batch_or_map, intrinsics, pose6, image_obs, R_base_camera=None, t_base_camera=None,
                              view_cfg=None, cfg: Optional[PhotometricEvidenceConfig] = None, chart_id: str = GC_CHART_ID,
                              anchor_id: str = "photometric_pose_evidence"
                              ) -> Tuple[PhotometricPoseEvidenceResult, CertBundle, ExpectedEffect]:
    """The operator for one linearisation pose [t, rotvec]: (PhotometricPoseEvidenceResult, CertBundle,
    ExpectedEffect). The certificate is approximate (triggers linearization and render_photometric_residual,
    support = (sum of the used pixels' coverage, n_used / (H W)), lift_strength = eps_lift), and exact when
    no pixel is used (L6 = 0, h = 0)."""
    cfg = cfg or PhotometricEvidenceConfig()
    pose = np.asarray(pose6, np.float64).ravel()[:6]
    Lp, hp, parts, render = photometric_pose_evidence_batched(batch_or_map, intrinsics, pose[None], image_obs, R_base_camera,
                                                              t_base_camera, view_cfg, cfg)
    return result_from_parts(Lp[0], hp[0], parts[0], render["alpha"].shape[1:], cfg.eps_lift, chart_id, anchor_id)
