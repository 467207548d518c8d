"""The one host driver of the pose evidences of the camera view ("Depth pose evidence" and
"Photometric pose evidence"), and what their results share, declared once.

prepare checks every argument before a device is asked for and makes what the three C entries read: the
splats (gc_camera_splat_prep), their tangents (gc_camera_splat_jvp, and gc_camera_shade_jvp with a luminance
channel), the tile lists and the forward raster (gc_render_depth_tiles), and the entries' argument tuples.
evidence allocates the outputs and calls the entry (evidence_call). No wait between the device calls; device
poses are read once before the first. A channel is (observation, configuration): DepthEvidenceConfig and
PhotometricEvidenceConfig check themselves (check)."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, Optional, Tuple

import numpy as np

from .. import _abi, rendering
from ..certificates import CertBundle, ExpectedEffect, InfluenceCert, SupportCert
from ..constants import D_Z, GC_CHART_ID, GC_EPS_LIFT
from .camera_features import DEPTH_MODELS, depth_image, image_shape
from .camera_splats import PinholeIntrinsics

MAX_POSES = _abi.GC_RENDER_MAX_VIEWS
MAX_TILE = 16  # a thread owns one pixel
ENTRIES = {"depth": "gc_depth_pose_evidence", "photo": "gc_photo_pose_evidence", "rgbd": "gc_rgbd_pose_evidence"}


@dataclass
class PoseEvidenceResult:
    L_pose: np.ndarray  # (22, 22)
    h_pose: np.ndarray  # (22,)
    L6: np.ndarray      # (6, 6) sum w J J^T, without the lift
    h6: np.ndarray      # (6,)
    total_weighted_cost: float
    n_used: int
    sum_coverage: float
    sum_weight: float


def parts_row_reader(result_cls, operator: str, trigger: str):
    """result_from_parts of an operator: one parts row [L6 (36) | h6 (6) | cost | n_used | sum_cov | sum_w] as
    (result_cls, CertBundle, ExpectedEffect). The certificate is approximate (triggers linearization and
    `trigger`, support = (sum of the used pixels' coverage, n_used / (H W)), lift_strength = eps_lift), and
    exact when no pixel is used."""
    def result_from_parts(L_pose, h_pose, parts, image_shape, eps_lift: float = GC_EPS_LIFT, chart_id: str = GC_CHART_ID,
                          anchor_id: str = operator):
        p = np.asarray(parts, np.float64)
        cost, n_used, sum_cov, sum_w = float(p[42]), int(p[43]), float(p[44]), float(p[45])
        result = result_cls(L_pose=L_pose, h_pose=h_pose, L6=p[0:36].reshape(6, 6).copy(), h6=p[36:42].copy(),
                            total_weighted_cost=cost, n_used=n_used, sum_coverage=sum_cov, sum_weight=sum_w)
        if n_used == 0:
            return (result, CertBundle.create_exact(chart_id=chart_id, anchor_id=anchor_id),
                    ExpectedEffect(objective_name=operator, predicted=0.0, realized=0.0))
        H, W = image_shape
        cert = CertBundle.create_approx(
            chart_id=chart_id, anchor_id=anchor_id, triggers=["linearization", trigger], frobenius_applied=False,
            support=SupportCert(ess_total=sum_cov, support_frac=n_used / float(H * W)),
            influence=InfluenceCert.identity().with_overrides(lift_strength=eps_lift))
        return result, cert, ExpectedEffect(objective_name=operator, predicted=cost, realized=cost)
    result_from_parts.__doc__ = f"One {operator} parts row as ({result_cls.__name__}, CertBundle, ExpectedEffect)."
    return result_from_parts


def _check_frame(intrinsics, poses6, R_base_camera, t_base_camera, view_cfg, what: str):
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


def image_obs(image, what: str = "image_obs"):
    """(H, W, is_rgb, image) of an observed image: (H, W, 3) uint8 rgb, or an (H, W) float luminance (NaN
    marks a hole; float32 is what the device reads). A DeviceArray is taken as it is."""
    sh = tuple(int(v) for v in (image.shape if isinstance(image, _abi.DeviceArray) else np.shape(image)))
    if len(sh) == 3:
        H, W, _ = image_shape(image, what, 3)
        dt = image.dtype if isinstance(image, _abi.DeviceArray) else np.asarray(image).dtype
        if dt != np.uint8:
            raise ValueError(f"{what} of shape {sh} and dtype {dt}: an rgb image is uint8")
        return H, W, True, image if isinstance(image, _abi.DeviceArray) else np.ascontiguousarray(image, np.uint8)
    H, W = image_shape(image, what, None)
    if isinstance(image, _abi.DeviceArray):
        if image.dtype != np.float32:
            raise ValueError(f"device {what} of dtype {image.dtype}, expected float32 luminance or uint8 rgb")
        return H, W, False, image
    a = np.asarray(image)
    if a.dtype.kind != "f":
        raise ValueError(f"{what} of shape {sh} and dtype {a.dtype}: a luminance image is float, an rgb image (H, W, 3)")
    return H, W, False, np.ascontiguousarray(a, np.float32)


def luminance_device(ctx, rgb, H: int, W: int, w: np.ndarray) -> _abi.DeviceArray:
    d_rgb = rgb if isinstance(rgb, _abi.DeviceArray) else _abi.DeviceArray.from_host(ctx, rgb, np.uint8)
    d_lum = _abi.DeviceArray(ctx, (H, W), np.float32)
    _abi.call("gc_image_luminance", ctx.handle, d_rgb.ptr, H, W, w.ctypes.data, d_lum.ptr, ctx=ctx)
    return d_lum


def prepare(batch_or_map, intrinsics, poses6, depth: Optional[Tuple], photo: Optional[Tuple], R_base_camera=None,
            t_base_camera=None, view_cfg=None, accumulate_into=None) -> SimpleNamespace:
    """The first half, for the depth channel depth = (depth_obs, DepthEvidenceConfig), the luminance channel
    photo = (image_obs, PhotometricEvidenceConfig) or both: the checked frame (ctx, P, n, H, W, eps_lift,
    accumulate_into, weights), render (the DeviceArrays made so far, under the names the callers get) and
    the argument tuples in the C entries' order: views (of the two jvp entries), st, frame, d_args and y_args
    (None without the channel). keep holds what their pointers point into."""
    view_cfg = view_cfg or rendering.CameraViewConfig()
    has_d, has_y = depth is not None, photo is not None
    what = "the RGB-D evidence" if has_d and has_y else "the depth evidence" if has_d else "the photometric evidence"
    P, host, Rbc, tbc = _check_frame(intrinsics, poses6, R_base_camera, t_base_camera, view_cfg, what)
    H = W = w = None
    if has_d:
        depth_obs, depth_cfg = depth
        depth_cfg.check()
        H, W, depth_obs = depth_image(depth_obs, "depth_obs")
    if has_y:
        obs, photo_cfg = photo
        w = photo_cfg.check()
        Hy, Wy, is_rgb, obs = image_obs(obs)
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
        render["depth_obs"] = depth_obs if isinstance(depth_obs, _abi.DeviceArray) else \
            _abi.DeviceArray.from_host(ctx, depth_obs, np.float32)
    if has_y:
        if is_rgb:
            render["lum_obs"] = luminance_device(ctx, obs, H, W, w)
        else:
            render["lum_obs"] = obs if isinstance(obs, _abi.DeviceArray) else _abi.DeviceArray.from_host(ctx, obs, np.float32)

    splats = rendering.camera_splat_prep(batch, Ks, T_cw, H, W, view_cfg)
    st = rendering._CamSplatStruct(*[splats[k].ptr for k, _ in rendering._CamSplatStruct._fields_])
    dm, dz, dS = _abi.alloc_many(ctx, [(P, n, 6, 2), (P, n, 6), (P, n, 6, 3)])
    views = (C.byref(batch.struct), n, P, T_cw.ctypes.data, t_wb.ctypes.data, K.ctypes.data, H, W, C.byref(c_cfg), C.byref(st))
    _abi.call("gc_camera_splat_jvp", ctx.handle, *views, dm.ptr, dz.ptr, dS.ptr, ctx=ctx)
    render.update(dmeans_px=dm, ddepths=dz, dSigmas_inv=dS)
    if has_y:
        dl, ddl = _abi.alloc_many(ctx, [(P, n), (P, n, 6)])
        _abi.call("gc_camera_shade_jvp", ctx.handle, *views, w.ctypes.data, dl.ptr, ddl.ptr, ctx=ctx)
        render.update(lum=dl, dlum=ddl)
    dev = rendering.render_depth_tiles(splats, H, W, view_cfg, ctx=ctx)
    frame = (H, W, ts, cap, C.byref(c_cfg), dev["tile_counts"].ptr, dev["tile_indices"].ptr, dev["alpha"].ptr)
    d_args = y_args = None
    if has_d:
        d_args = (dev["depth"].ptr, render["depth_obs"].ptr, DEPTH_MODELS.index(depth_cfg.depth_model),
                  float(depth_cfg.depth_sigma0), float(depth_cfg.depth_sigma_slope), float(depth_cfg.min_depth_m),
                  float(depth_cfg.max_depth_m), int(depth_cfg.robust_nu is not None), float(depth_cfg.robust_nu or 0.0))
    if has_y:
        y_args = (render["lum_obs"].ptr, float(photo_cfg.sigma), int(photo_cfg.robust_nu is not None),
                  float(photo_cfg.robust_nu or 0.0))
    return SimpleNamespace(ctx=ctx, P=P, n=n, H=H, W=W, eps_lift=eps_lift, accumulate_into=accumulate_into, weights=w,
                           render=dict(dev, **splats, **render), views=views, st=st, frame=frame, d_args=d_args,
                           y_args=y_args, keep=(batch, T_cw, t_wb, K, c_cfg))


def evidence_call(f, kind: str, accumulate, dL, dh, dparts, images=None):
    """One C entry (ENTRIES[kind]) on a prepared view; images: the entry's optional image outputs in its
    order (two of depth, three of photo, five of rgbd), None for none."""
    d, y = kind != "photo", kind != "depth"
    r = f.render
    tangents = [r["dmeans_px"]] + ([r["ddepths"]] if d else []) + [r["dSigmas_inv"]] + ([r["lum"], r["dlum"]] if y else [])
    images = images or [None] * (2 * d + 3 * y)
    _abi.call(ENTRIES[kind], f.ctx.handle, f.P, f.n, C.byref(f.st), *[t.ptr for t in tangents], *f.frame,
              *(f.d_args if d else ()), *(f.y_args if y else ()), f.eps_lift, int(accumulate), dL.ptr, dh.ptr, dparts.ptr,
              *[i.ptr if i is not None else None for i in images], ctx=f.ctx)


def evidence(f, device_out: bool = False, return_images: bool = False, joint: bool = True):
    """The second half: (L_pose, h_pose, parts, render) of the prepared channels. With both, joint chooses the
    one-pass entry or the depth entry followed by the luminance entry; the bytes are the same."""
    ctx, P, into = f.ctx, f.P, f.accumulate_into
    has_d, has_y = f.d_args is not None, f.y_args is not None
    pshape = (P, 2, _abi.GC_DEPTHEV_PARTS) if has_d and has_y else (P, _abi.GC_DEPTHEV_PARTS)
    if into is not None:
        dL = _abi.device_input(ctx, into[0], np.float64, (P, D_Z, D_Z))
        dh = _abi.device_input(ctx, into[1], np.float64, (P, D_Z))
        (dparts,) = _abi.alloc_many(ctx, [pshape])
    else:
        dL, dh, dparts = _abi.alloc_many(ctx, [(P, D_Z, D_Z), (P, D_Z), pshape])
    names, imgs = [], None
    if return_images:
        names = (["residual", "weight"] if has_d else []) + \
                ((["lum_render", "lum_residual", "lum_weight"] if has_d else ["lum_render", "residual", "weight"]) if has_y else [])
        imgs = _abi.alloc_many(ctx, [(P, f.H, f.W)] * len(names))
    acc = into is not None
    if has_d and has_y and not joint:  # the same bytes from the two entries: the depth's row and sums, then the luminance's added
        dparts = tuple(_abi.alloc_many(ctx, [(P, _abi.GC_DEPTHEV_PARTS)] * 2))
        evidence_call(f, "depth", acc, dL, dh, dparts[0], imgs and imgs[:2])
        evidence_call(f, "photo", True, dL, dh, dparts[1], imgs and imgs[2:])
    else:
        evidence_call(f, "rgbd" if has_d and has_y else "depth" if has_d else "photo", acc, dL, dh, dparts, imgs)
    render = dict(f.render, **dict(zip(names, imgs or ())))

    def parts_host():
        if isinstance(dparts, tuple):
            return np.stack(_abi.download_many(list(dparts)), axis=1)
        return dparts.download()

    if device_out:
        return dL, dh, parts_host(), render
    if into is None and not isinstance(dparts, tuple):
        Lp, hp, parts = _abi.download_many([dL, dh, dparts])
        return Lp.copy(), hp.copy(), parts.copy(), render
    return dL.download(), dh.download(), parts_host(), render
