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

Every argument error is raised here before a device is asked for; the device calls run with no wait
between them."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np

from .. import _abi, rendering
from ..certificates import CertBundle, ExpectedEffect, InfluenceCert, SupportCert
from ..constants import D_Z, GC_CHART_ID, GC_EPS_LIFT
from .camera_features import DEPTH_MODELS, _depth_image, _image_shape
from .depth_pose_evidence import DepthEvidenceConfig, _check_accumulate, _check_frame
from .depth_pose_evidence import _check_cfg as _check_depth_cfg

GREY_WEIGHTS = (4899.0 / 16384.0, 9617.0 / 16384.0, 1868.0 / 16384.0)  # the keypoint detector's grey

# Whether rgbd_pose_evidence_batched makes the one joint call (gc_rgbd_pose_evidence) or the depth call and
# then the luminance call, when the caller does not say: the bytes are the same either way, the choice is
# the measured one. The joint entry's median is below the two single entries' sum by more than the two
# p10-p90 spreads together in all four shapes of tools/probe/time_photo_evidence.py (DESIGN.md §4,
# "Photometric pose evidence", measured times).
RGBD_JOINT_DEFAULT = True


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


@dataclass
class PhotometricPoseEvidenceResult:
    L_pose: np.ndarray  # (22, 22)
    h_pose: np.ndarray  # (22,)
    L6: np.ndarray      # (6, 6) sum w J J^T, without the lift
    h6: np.ndarray      # (6,)
    total_weighted_cost: float
    n_used: int
    sum_coverage: float
    sum_weight: float


def _weights(weights) -> np.ndarray:
    try:
        w = np.ascontiguousarray(GREY_WEIGHTS if weights is None else weights, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"weights must hold 3 finite values, got {weights!r}") from None
    if w.shape != (3,) or not np.isfinite(w).all():
        raise ValueError(f"weights must hold 3 finite values, got {weights!r}")
    return w


def _check_cfg(cfg: PhotometricEvidenceConfig) -> np.ndarray:
    w = _weights(cfg.weights)
    vals = [cfg.sigma, cfg.eps_lift] + ([] if cfg.robust_nu is None else [cfg.robust_nu])
    if not np.isfinite(np.asarray(vals, np.float64)).all():
        raise ValueError("the photometric evidence configuration must be finite")
    if not cfg.sigma > 0.0:
        raise ValueError(f"sigma must be > 0, got {cfg.sigma}")
    if cfg.robust_nu is not None and not cfg.robust_nu > 0.0:
        raise ValueError(f"robust_nu must be > 0 or None, got {cfg.robust_nu}")
    if cfg.eps_lift < 0.0:
        raise ValueError(f"eps_lift must be >= 0, got {cfg.eps_lift}")
    return w


def _image_obs(image, what: str = "image_obs"):
    """(H, W, is_rgb, image) of an observed image: (H, W, 3) uint8 rgb, or an (H, W) float luminance (NaN
    marks a hole; float32 is what the device reads). A DeviceArray is taken as it is."""
    sh = tuple(int(v) for v in (image.shape if isinstance(image, _abi.DeviceArray) else np.shape(image)))
    if len(sh) == 3:
        H, W, _ = _image_shape(image, what, 3)
        dt = image.dtype if isinstance(image, _abi.DeviceArray) else np.asarray(image).dtype
        if dt != np.uint8:
            raise ValueError(f"{what} of shape {sh} and dtype {dt}: an rgb image is uint8")
        return H, W, True, image if isinstance(image, _abi.DeviceArray) else np.ascontiguousarray(image, np.uint8)
    H, W = _image_shape(image, what, None)
    if isinstance(image, _abi.DeviceArray):
        if image.dtype != np.float32:
            raise ValueError(f"device {what} of dtype {image.dtype}, expected float32 luminance or uint8 rgb")
        return H, W, False, image
    a = np.asarray(image)
    if a.dtype.kind != "f":
        raise ValueError(f"{what} of shape {sh} and dtype {a.dtype}: a luminance image is float, an rgb image (H, W, 3)")
    return H, W, False, np.ascontiguousarray(a, np.float32)


def _luminance_device(ctx, rgb, H: int, W: int, w: np.ndarray) -> _abi.DeviceArray:
    d_rgb = rgb if isinstance(rgb, _abi.DeviceArray) else _abi.DeviceArray.from_host(ctx, rgb, np.uint8)
    d_lum = _abi.DeviceArray(ctx, (H, W), np.float32)
    _abi.call("gc_image_luminance", ctx.handle, d_rgb.ptr, H, W, w.ctypes.data, d_lum.ptr, ctx=ctx)
    return d_lum


def luminance_image(rgb, weights=None, *, ctx=None, device_out: bool = False):
    """An (H, W, 3) uint8 rgb image (host or DeviceArray) as the float32 luminance
    ((w_r R + w_g G) + w_b B) / 255, summed in f64 (gc_image_luminance): what the evidence observes."""
    w = _weights(weights)
    H, W, is_rgb, img = _image_obs(rgb, "rgb")
    if not is_rgb:
        raise ValueError(f"rgb of shape {(H, W)}, expected (H, W, 3)")
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise ValueError(f"H and W must be in [1, 16384], got {H}, {W}")
    ctx = ctx or (img.ctx if isinstance(img, _abi.DeviceArray) else _abi.default_context())
    d = _luminance_device(ctx, img, H, W, w)
    return d if device_out else d.download()


def _run(batch_or_map, intrinsics, poses6, depth_obs, image_obs, R_base_camera, t_base_camera, view_cfg, depth_cfg,
         photo_cfg, accumulate_into, device_out: bool, return_images: bool, joint: Optional[bool]):
    """The depth evidence (depth_obs given), the photometric evidence (image_obs given) or both, from one prep,
    one set of tile lists and one forward raster."""
    view_cfg = view_cfg or rendering.CameraViewConfig()
    has_d, has_y = depth_obs is not None, image_obs is not None
    what = "the photometric evidence" if not has_d else "the RGB-D evidence"
    P, host, Rbc, tbc = _check_frame(intrinsics, poses6, R_base_camera, t_base_camera, view_cfg, what)
    H = W = None
    if has_d:
        depth_cfg = depth_cfg or DepthEvidenceConfig()
        _check_depth_cfg(depth_cfg)
        H, W, depth_obs = _depth_image(depth_obs, "depth_obs")
    if has_y:
        photo_cfg = photo_cfg or PhotometricEvidenceConfig()
        w = _check_cfg(photo_cfg)
        Hy, Wy, is_rgb, image_obs = _image_obs(image_obs)
        if has_d and (Hy, Wy) != (H, W):
            raise ValueError(f"image_obs of {Hy} x {Wy} pixels beside depth_obs of {H} x {W}")
        H, W = Hy, Wy
    if has_d and has_y and depth_cfg.eps_lift != photo_cfg.eps_lift:
        raise ValueError(f"one lift is added: depth_cfg.eps_lift = {depth_cfg.eps_lift} and photo_cfg.eps_lift = "
                         f"{photo_cfg.eps_lift} must agree")
    eps_lift = float((depth_cfg if has_d else photo_cfg).eps_lift)
    rendering._check_camera_args(intrinsics, np.eye(4), H, W, view_cfg, 0)
    _check_accumulate(accumulate_into, P)
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
    render: Dict[str, _abi.DeviceArray] = {}
    if has_d:
        d_obs = depth_obs if isinstance(depth_obs, _abi.DeviceArray) else _abi.DeviceArray.from_host(ctx, depth_obs, np.float32)
        render["depth_obs"] = d_obs
    if has_y:
        if is_rgb:
            d_lobs = _luminance_device(ctx, image_obs, H, W, w)
        else:
            d_lobs = image_obs if isinstance(image_obs, _abi.DeviceArray) else _abi.DeviceArray.from_host(ctx, image_obs, np.float32)
        render["lum_obs"] = d_lobs

    splats = rendering.camera_splat_prep(batch, Ks, T_cw, H, W, view_cfg)
    st = rendering._CamSplatStruct(*[splats[k].ptr for k, _ in rendering._CamSplatStruct._fields_])
    dm, dz, dS = _abi.alloc_many(ctx, [(P, n, 6, 2), (P, n, 6), (P, n, 6, 3)])
    views = (T_cw.ctypes.data, t_wb.ctypes.data, K.ctypes.data, H, W, C.byref(c_cfg), C.byref(st))
    _abi.call("gc_camera_splat_jvp", ctx.handle, C.byref(batch.struct), n, P, *views, dm.ptr, dz.ptr, dS.ptr, ctx=ctx)
    render.update(dmeans_px=dm, ddepths=dz, dSigmas_inv=dS)
    if has_y:
        dl, ddl = _abi.alloc_many(ctx, [(P, n), (P, n, 6)])
        _abi.call("gc_camera_shade_jvp", ctx.handle, C.byref(batch.struct), n, P, *views, w.ctypes.data, dl.ptr, ddl.ptr,
                  ctx=ctx)
        render.update(lum=dl, dlum=ddl)
    dev = rendering.render_depth_tiles(splats, H, W, view_cfg, ctx=ctx)
    rows = 2 if (has_d and has_y) else 1
    pshape = (P, 2, _abi.GC_DEPTHEV_PARTS) if rows == 2 else (P, _abi.GC_DEPTHEV_PARTS)
    if accumulate_into is not None:
        dL = _abi.device_input(ctx, accumulate_into[0], np.float64, (P, D_Z, D_Z))
        dh = _abi.device_input(ctx, accumulate_into[1], np.float64, (P, D_Z))
        (dparts,) = _abi.alloc_many(ctx, [pshape])
    else:
        dL, dh, dparts = _abi.alloc_many(ctx, [(P, D_Z, D_Z), (P, D_Z), pshape])
    img = {}
    if return_images:
        names = (["residual", "weight"] if has_d else []) + \
                ((["lum_render", "lum_residual", "lum_weight"] if has_d else ["lum_render", "residual", "weight"]) if has_y else [])
        img = dict(zip(names, _abi.alloc_many(ctx, [(P, H, W)] * len(names))))
    ip = lambda k: img[k].ptr if k in img else None
    acc = int(accumulate_into is not None)
    frame = (H, W, ts, cap, C.byref(c_cfg), dev["tile_counts"].ptr, dev["tile_indices"].ptr, dev["alpha"].ptr)
    if has_d:
        d_args = (dev["depth"].ptr, d_obs.ptr, DEPTH_MODELS.index(depth_cfg.depth_model), float(depth_cfg.depth_sigma0),
                  float(depth_cfg.depth_sigma_slope), float(depth_cfg.min_depth_m), float(depth_cfg.max_depth_m),
                  int(depth_cfg.robust_nu is not None), float(depth_cfg.robust_nu or 0.0))
    if has_y:
        y_args = (d_lobs.ptr, float(photo_cfg.sigma), int(photo_cfg.robust_nu is not None), float(photo_cfg.robust_nu or 0.0))
    if rows == 2 and (RGBD_JOINT_DEFAULT if joint is None else joint):
        _abi.call("gc_rgbd_pose_evidence", ctx.handle, P, n, C.byref(st), dm.ptr, dz.ptr, dS.ptr, dl.ptr, ddl.ptr, *frame,
                  *d_args, *y_args, eps_lift, acc, dL.ptr, dh.ptr, dparts.ptr, ip("residual"), ip("weight"),
                  ip("lum_render"), ip("lum_residual"), ip("lum_weight"), ctx=ctx)
    elif rows == 2:  # the same bytes from the two entries: the depth's row and sums, then the luminance's added
        pd, py = _abi.alloc_many(ctx, [(P, _abi.GC_DEPTHEV_PARTS)] * 2)
        _abi.call("gc_depth_pose_evidence", ctx.handle, P, n, C.byref(st), dm.ptr, dz.ptr, dS.ptr, *frame, *d_args,
                  eps_lift, acc, dL.ptr, dh.ptr, pd.ptr, ip("residual"), ip("weight"), ctx=ctx)
        _abi.call("gc_photo_pose_evidence", ctx.handle, P, n, C.byref(st), dm.ptr, dS.ptr, dl.ptr, ddl.ptr, *frame, *y_args,
                  eps_lift, 1, dL.ptr, dh.ptr, py.ptr, ip("lum_render"), ip("lum_residual"), ip("lum_weight"), ctx=ctx)
        dparts = (pd, py)
    elif has_d:
        _abi.call("gc_depth_pose_evidence", ctx.handle, P, n, C.byref(st), dm.ptr, dz.ptr, dS.ptr, *frame, *d_args,
                  eps_lift, acc, dL.ptr, dh.ptr, dparts.ptr, ip("residual"), ip("weight"), ctx=ctx)
    else:
        _abi.call("gc_photo_pose_evidence", ctx.handle, P, n, C.byref(st), dm.ptr, dS.ptr, dl.ptr, ddl.ptr, *frame, *y_args,
                  eps_lift, acc, dL.ptr, dh.ptr, dparts.ptr, ip("lum_render"), ip("residual"), ip("weight"), ctx=ctx)
    render = dict(dev, **splats, **render, **img)

    def parts_host():
        if isinstance(dparts, tuple):
            return np.stack(_abi.download_many(list(dparts)), axis=1)
        return dparts.download()

    if device_out:
        return dL, dh, parts_host(), render
    if accumulate_into is None and not isinstance(dparts, tuple):
        Lp, hp, parts = _abi.download_many([dL, dh, dparts])
        return Lp.copy(), hp.copy(), parts.copy(), render
    return dL.download(), dh.download(), parts_host(), render


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
    return _run(batch_or_map, intrinsics, poses6, None, image_obs, R_base_camera, t_base_camera, view_cfg, None, cfg,
                accumulate_into, device_out, return_images, None)


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
    return _run(batch_or_map, intrinsics, poses6, depth_obs, image_obs, R_base_camera, t_base_camera, view_cfg, depth_cfg,
                photo_cfg, accumulate_into, device_out, return_images, joint)


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


def result_from_parts(L_pose, h_pose, parts, image_shape, eps_lift: float = GC_EPS_LIFT, chart_id: str = GC_CHART_ID,
                      anchor_id: str = "photometric_pose_evidence"):
    """One luminance parts row as (PhotometricPoseEvidenceResult, CertBundle, ExpectedEffect)."""
    p = np.asarray(parts, np.float64)
    cost, n_used, sum_cov, sum_w = float(p[42]), int(p[43]), float(p[44]), float(p[45])
    result = PhotometricPoseEvidenceResult(L_pose=L_pose, h_pose=h_pose, L6=p[0:36].reshape(6, 6).copy(), h6=p[36:42].copy(),
                                           total_weighted_cost=cost, n_used=n_used, sum_coverage=sum_cov, sum_weight=sum_w)
    if n_used == 0:
        return (result, CertBundle.create_exact(chart_id=chart_id, anchor_id=anchor_id),
                ExpectedEffect(objective_name="photometric_pose_evidence", predicted=0.0, realized=0.0))
    H, W = image_shape
    cert = CertBundle.create_approx(
        chart_id=chart_id, anchor_id=anchor_id, triggers=["linearization", "render_photometric_residual"],
        frobenius_applied=False, support=SupportCert(ess_total=sum_cov, support_frac=n_used / float(H * W)),
        influence=InfluenceCert.identity().with_overrides(lift_strength=eps_lift))
    return result, cert, ExpectedEffect(objective_name="photometric_pose_evidence", predicted=cost, realized=cost)
