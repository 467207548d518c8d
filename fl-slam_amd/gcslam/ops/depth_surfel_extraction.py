"""RGB-D surfel extraction on the GPU ("Depth surfels"): one depth image and, optionally, its
rgb image -> coloured rows of the camera slice (sources = 0) of a MeasurementBatch, in the base frame. The
depth image is cut into cell_px x cell_px cells, every cell gets the LiDAR extractor's plane fit
(lidar_surfel_extraction.py:84-163 from the covariance on, with sigma_z(zbar)^2 as the sensor's variance) and
the cell's mean colour, and the valid cells, thinned evenly when they outnumber the free camera rows, are
written in information form with one vMF lobe. The operator is this build's: the reference's camera path is
ORB-only. Its semantics are stated at gc_extract_depth_surfels in include/gcslam.h; all arithmetic runs in
libgcslam (csrc/gc_depthsurfel.hip)."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .. import _abi
from ..certificates import CertBundle, ExpectedEffect, InfluenceCert, SupportCert
from ..constants import GC_CHART_ID, GC_EPS_LIFT, GC_N_FEAT, GC_N_SURFEL, GC_VMF_N_LOBES
from ..measurement_batch import BATCH_ARRAYS, MeasurementBatch
from ..rendering import _extrinsics
from .camera_features import DEPTH_MODELS, depth_image, image_shape
from .camera_splats import PinholeIntrinsics

MIN_CELL, MAX_CELL = 4, 32  # gc_depthsurfel.hip: one wave per cell, at most 16 pixels per lane
MAX_AXIS = 16384


@dataclass
class DepthSurfelConfig:
    """The depth model and limits are VisualFeatureConfig's and DepthEvidenceConfig's under the same names; the
    budgets, the Wishart prior, kappa, eig_min and eps_lift are SurfelExtractionConfig's. The cell size and
    the gates (min_fill, plane_gate, min_cos_incidence) and weight_scale are this build's choices, not the
    reference's: a cell needs half its pixels, a plane residual within two depth sigmas, and a surface seen
    at more than about 6 degrees off edge-on."""
    cell_px: int = 16
    min_fill: float = 0.5
    min_depth_m: float = 0.05
    max_depth_m: float = 80.0
    depth_model: str = "linear"
    depth_sigma0: float = 0.01
    depth_sigma_slope: float = 0.01
    plane_gate: float = 2.0
    min_cos_incidence: float = 0.1
    weight_scale: float = 1.0
    n_surfel: int = GC_N_SURFEL
    n_feat: int = GC_N_FEAT
    wishart_nu: float = 5.0
    wishart_psi_scale: float = 0.1
    kappa_main_scale: float = 10.0
    kappa_min: float = 0.1
    kappa_max: float = 100.0
    eig_min: float = 1e-12
    eps_lift: float = GC_EPS_LIFT

    def check(self):
        """Every configuration error the device entry would reject."""
        if self.depth_model not in DEPTH_MODELS:
            raise ValueError(f"Unknown depth_model: {self.depth_model!r}; one of {DEPTH_MODELS}")
        vals = [self.cell_px, self.min_fill, self.min_depth_m, self.max_depth_m, self.depth_sigma0,
                self.depth_sigma_slope, self.plane_gate, self.min_cos_incidence, self.weight_scale, self.n_surfel,
                self.n_feat, self.wishart_nu, self.wishart_psi_scale, self.kappa_main_scale, self.kappa_min,
                self.kappa_max, self.eig_min, self.eps_lift]
        if not np.isfinite(np.asarray(vals, np.float64)).all():
            raise ValueError("the depth surfel configuration must be finite")
        if int(self.cell_px) != self.cell_px or not MIN_CELL <= self.cell_px <= MAX_CELL:
            raise ValueError(f"cell_px must be an integer in [{MIN_CELL}, {MAX_CELL}], got {self.cell_px}")
        if int(self.n_feat) != self.n_feat or self.n_feat < 0:
            raise ValueError(f"n_feat must be a non-negative integer, got {self.n_feat}")
        if int(self.n_surfel) != self.n_surfel or self.n_surfel < 0:
            raise ValueError(f"n_surfel must be a non-negative integer, got {self.n_surfel}")
        if not 0.0 < self.min_fill <= 1.0:
            raise ValueError(f"min_fill must be in (0, 1], got {self.min_fill}")
        if not 0.0 <= self.min_depth_m < self.max_depth_m:
            raise ValueError(f"the depth limits must satisfy 0 <= min_depth_m < max_depth_m, got {self.min_depth_m}, "
                             f"{self.max_depth_m}")
        if not (self.depth_sigma0 > 0.0 and self.depth_sigma_slope >= 0.0):
            raise ValueError(f"depth_sigma0 must be > 0 and depth_sigma_slope >= 0, got {self.depth_sigma0}, "
                             f"{self.depth_sigma_slope}")
        if not self.plane_gate > 0.0:
            raise ValueError(f"plane_gate must be > 0, got {self.plane_gate}")
        if not 0.0 <= self.min_cos_incidence < 1.0:
            raise ValueError(f"min_cos_incidence must be in [0, 1), got {self.min_cos_incidence}")


def _validate(depth, rgb, intrinsics, R_base_camera, t_base_camera, timestamp_sec, cfg: DepthSurfelConfig, base_batch):
    """Every argument error, raised before a context or a launch: (H, W, depth, rgb, K, Rbc, tbc, n_lobes)."""
    cfg.check()
    if not isinstance(intrinsics, PinholeIntrinsics):
        raise ValueError("intrinsics must be a PinholeIntrinsics")
    K = np.array([intrinsics.fx, intrinsics.fy, intrinsics.cx, intrinsics.cy], np.float64)
    if not np.isfinite(K).all() or K[0] == 0.0 or K[1] == 0.0:
        raise ValueError(f"the intrinsics must be finite with fx, fy != 0, got {K}")
    H, W, depth = depth_image(depth, "depth")
    if not (1 <= H <= MAX_AXIS and 1 <= W <= MAX_AXIS):
        raise ValueError(f"depth of {H} x {W} pixels: H and W must be in [1, {MAX_AXIS}]")
    if H * W > _abi.GC_IMAGE_MAX_PIXELS:
        raise ValueError(f"depth of {H} x {W} pixels: at most {_abi.GC_IMAGE_MAX_PIXELS} are supported")
    cell = int(cfg.cell_px)
    n_cells = (-(-H // cell)) * (-(-W // cell))
    if n_cells > _abi.GC_SURFEL_MAX_CELLS:
        raise ValueError(f"the image holds {n_cells} cells of {cell} px; at most {_abi.GC_SURFEL_MAX_CELLS} are supported")
    if rgb is not None:
        if image_shape(rgb, "rgb", 3)[:2] != (H, W):
            raise ValueError(f"rgb of shape {tuple(rgb.shape)} beside depth of {H} x {W} pixels")
        dt = rgb.dtype if isinstance(rgb, _abi.DeviceArray) else np.asarray(rgb).dtype
        if dt != np.uint8:
            raise ValueError(f"rgb of dtype {dt}, expected uint8")
        if not isinstance(rgb, _abi.DeviceArray):
            rgb = np.ascontiguousarray(rgb, np.uint8)
    Rbc, tbc = _extrinsics(R_base_camera, t_base_camera)
    if not (np.isfinite(Rbc).all() and np.isfinite(tbc).all()):
        raise ValueError("the extrinsics must be finite")
    if not np.isfinite(float(timestamp_sec)):
        raise ValueError(f"timestamp_sec must be finite, got {timestamp_sec}")
    n_lobes = GC_VMF_N_LOBES
    if base_batch is not None:
        if int(base_batch.n_feat) != int(cfg.n_feat) or int(base_batch.n_surfel) != int(cfg.n_surfel):
            raise ValueError(f"base_batch budgets (n_feat {base_batch.n_feat}, n_surfel {base_batch.n_surfel}) differ "
                             f"from the config's ({cfg.n_feat}, {cfg.n_surfel})")
        n_total = int(cfg.n_feat) + int(cfg.n_surfel)
        esh = tuple(base_batch.etas.shape)
        if len(esh) != 3 or esh[0] != n_total or esh[2] != 3 or not 1 <= esh[1] <= 8:
            raise ValueError(f"base_batch.etas of shape {esh}, expected ({n_total}, n_lobes, 3)")
        n_lobes = int(esh[1])
        if not 0 <= int(base_batch.n_camera_valid) <= int(cfg.n_feat):
            raise ValueError(f"base_batch.n_camera_valid = {base_batch.n_camera_valid} outside [0, {cfg.n_feat}]")
    return H, W, depth, rgb, K, np.ascontiguousarray(Rbc), np.ascontiguousarray(tbc), n_lobes


def extract_depth_surfels(depth, rgb, intrinsics, R_base_camera=None, t_base_camera=None, timestamp_sec: float = 0.0,
                          config: Optional[DepthSurfelConfig] = None, base_batch: Optional[MeasurementBatch] = None,
                          chart_id: str = GC_CHART_ID, anchor_id: str = "depth_surfel_extraction", ctx=None,
                          device_out: bool = False) -> Tuple[MeasurementBatch, CertBundle, ExpectedEffect]:
    """depth (H, W; metres, float32) and rgb ((H, W, 3) uint8, or None: the rows take the LiDAR rows' grey) are
    host arrays or DeviceArrays; intrinsics a PinholeIntrinsics; the camera sits at the body when
    R_base_camera and t_base_camera are None. With base_batch every row of it is carried over (the camera
    rows below its n_camera_valid and the whole LiDAR slice included; host- or device-resident) and the new
    rows follow its camera rows: n_camera_valid = the base's + n_new, n_lidar_valid = the base's; otherwise
    the batch is zero elsewhere. With device_out the nine arrays stay in HBM: they are the batch's fields and
    batch.device. batch.depth_slot_cells (n_feat, int32) holds the image cell of every row written, -1
    elsewhere. The call waits once, for the row count."""
    cfg = config or DepthSurfelConfig()
    H, W, depth, rgb, K, Rbc, tbc, n_lobes = _validate(depth, rgb, intrinsics, R_base_camera, t_base_camera,
                                                       timestamp_sec, cfg, base_batch)
    n_feat, n_surfel = int(cfg.n_feat), int(cfg.n_surfel)
    n_total = n_feat + n_surfel
    n_in = int(base_batch.n_camera_valid) if base_batch is not None else 0
    ctx = ctx or _abi.default_context()
    dd = _abi.device_input(ctx, depth, np.float32, (H, W))
    dc = _abi.device_input(ctx, rgb, np.uint8, (H, W, 3)) if rgb is not None else None
    names = list(BATCH_ARRAYS)
    shapes = {k: (n_total,) + (shp if k != "etas" else (n_lobes, 3)) for k, (shp, _, _) in BATCH_ARRAYS.items()}
    # the nine arrays and the slot -> cell record as views of one block: one fill, one download
    blk = _abi.alloc_many(ctx, [(shapes[k], BATCH_ARRAYS[k][2]) for k in names] + [((n_feat,), np.int32)])
    out, d_cells = dict(zip(names, blk[:-1])), blk[-1]
    if base_batch is None:
        blk[0]._base.zero()
    else:
        src = getattr(base_batch, "device", None) or {}
        for k in names:
            s = src.get(k, getattr(base_batch, k))
            if isinstance(s, _abi.DeviceArray):
                s = _abi.device_input(ctx, s, BATCH_ARRAYS[k][2], shapes[k])
                _abi.call("gc_buffer_copy", ctx.handle, out[k].ptr, s.ptr, out[k].nbytes, ctx=ctx)
            else:
                out[k].upload(np.ascontiguousarray(s).reshape(shapes[k]).astype(BATCH_ARRAYS[k][2], copy=False))
    nv = C.c_int32(0)
    ignored = dict(voxel_size_m=0.0, hex3d_num_cells_1=0.0, hex3d_num_cells_2=0.0, hex3d_num_cells_z=0.0,
                   hex3d_max_occupants=0.0, min_points_per_voxel=0.0, sensor_noise_var_per_axis=0.0)
    _abi.call("gc_extract_depth_surfels", ctx.handle, dd.ptr, dc.ptr if dc is not None else None, H, W, K.ctypes.data,
              Rbc.ctypes.data, tbc.ctypes.data, float(timestamp_sec), n_in,
              C.byref(_abi.cfg("gc_surfel_cfg", cfg, n_lobes=n_lobes, **ignored)), int(cfg.cell_px), float(cfg.min_fill),
              float(cfg.min_depth_m), float(cfg.max_depth_m), DEPTH_MODELS.index(cfg.depth_model), float(cfg.depth_sigma0),
              float(cfg.depth_sigma_slope), float(cfg.plane_gate), float(cfg.min_cos_incidence), float(cfg.weight_scale),
              *[out[k].ptr for k in names], d_cells.ptr, C.byref(nv), ctx=ctx)
    n_new = int(nv.value)
    counts = dict(n_feat=n_feat, n_surfel=n_surfel, n_camera_valid=n_in + n_new,
                  n_lidar_valid=int(base_batch.n_lidar_valid) if base_batch is not None else 0)
    if device_out:
        batch = MeasurementBatch(**out, **counts, device=dict(out), depth_slot_cells=d_cells)
    else:
        host = dict(zip(names + ["cells"], _abi.download_many(blk)))
        cells = host.pop("cells")
        host = {k: v.astype(BATCH_ARRAYS[k][1], copy=False) for k, v in host.items()}
        batch = MeasurementBatch(**host, **counts, depth_slot_cells=cells)
    cert = CertBundle.create_approx(
        chart_id=chart_id, anchor_id=anchor_id,
        triggers=["depth_cell_binning", "plane_fit_batched", "wishart_regularization"],
        support=SupportCert(ess_total=float(n_new), support_frac=float(n_new) / float(max(n_feat - n_in, 1))),
        influence=InfluenceCert.identity())
    return batch, cert, ExpectedEffect(objective_name="depth_surfel_extraction", predicted=float(n_new),
                                       realized=float(n_new))
