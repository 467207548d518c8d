"""LiDAR surfel extraction (backend/operators/lidar_surfel_extraction.py:339-431) on the GPU: the
deskewed points of one scan -> the LiDAR slice of a MeasurementBatch. MA-hex 3D hash binning
(common/ma_hex_web.py:221-303), a weighted plane fit per cell with Wishart regularisation
(:84-163), the first n_surfel valid cells in ascending cell id (:297-321) written in information
form with one vMF lobe (structures/measurement_batch.py:262-347). The reference runs it on every
scan directly after the deskew and directly before the association (backend/pipeline.py:781-800);
all arithmetic runs in libgcslam (gc_extract_lidar_surfels, csrc/gc_surfel.hip)."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .. import _abi
from ..certificates import CertBundle, ExpectedEffect, InfluenceCert, SupportCert
from ..constants import GC_CHART_ID, GC_EPS_LIFT, GC_N_FEAT, GC_N_SURFEL, GC_VMF_N_LOBES
from ..measurement_batch import BATCH_ARRAYS, MeasurementBatch


@dataclass
class SurfelExtractionConfig:
    """lidar_surfel_extraction.py:43-62."""
    n_surfel: int = GC_N_SURFEL
    n_feat: int = GC_N_FEAT
    voxel_size_m: float = 0.1
    hex3d_num_cells_1: int = 32
    hex3d_num_cells_2: int = 32
    hex3d_num_cells_z: int = 8
    hex3d_max_occupants: int = 32
    min_points_per_voxel: int = 3
    sensor_noise_var_per_axis: float = 1e-6
    wishart_nu: float = 5.0
    wishart_psi_scale: float = 0.1
    kappa_main_scale: float = 10.0
    kappa_min: float = 0.1
    kappa_max: float = 100.0
    eig_min: float = 1e-12
    eps_lift: float = GC_EPS_LIFT


def _rows(x, width=1) -> int:
    sh = x.shape if isinstance(x, _abi.DeviceArray) else np.shape(x)
    n = int(np.prod(sh)) if sh else 1
    if n % width:
        raise ValueError(f"array of shape {tuple(sh)} does not hold rows of {width}")
    return n // width


def _validate(n: int, n_t: int, n_w: int, cfg: SurfelExtractionConfig, base_batch) -> None:
    """Every argument error the device entry would reject, raised before a context or a launch."""
    if n_t != n or n_w != n:
        raise ValueError(f"timestamps ({n_t}) / weights ({n_w}) must match the {n} points")
    grid = (cfg.hex3d_num_cells_1, cfg.hex3d_num_cells_2, cfg.hex3d_num_cells_z)
    if any(int(g) != g or g <= 0 for g in grid):
        raise ValueError(f"hex3d grid sizes must be positive integers, got {grid}")
    n_cells = int(grid[0]) * int(grid[1]) * int(grid[2])
    if n_cells > _abi.GC_SURFEL_MAX_CELLS:
        raise ValueError(f"the hash grid holds {n_cells} cells; the kernel supports at most "
                         f"{_abi.GC_SURFEL_MAX_CELLS} (cell keys below 2^14)")
    if int(cfg.n_surfel) != cfg.n_surfel or cfg.n_surfel <= 0:
        raise ValueError(f"n_surfel must be a positive integer, got {cfg.n_surfel}")
    if int(cfg.n_feat) != cfg.n_feat or cfg.n_feat < 0:
        raise ValueError(f"n_feat must be a non-negative integer, got {cfg.n_feat}")
    if not cfg.voxel_size_m > 0.0:
        raise ValueError(f"voxel_size_m must be > 0, got {cfg.voxel_size_m}")
    if 2e5 / float(cfg.voxel_size_m) >= 2.0 ** 31:
        raise ValueError(f"voxel_size_m = {cfg.voxel_size_m} is too small: the int32 cell index needs "
                         "2e5 / voxel_size_m < 2^31")
    occ = cfg.hex3d_max_occupants
    if int(occ) != occ or not 1 <= occ <= _abi.GC_SURFEL_MAX_OCCUPANTS:
        raise ValueError(f"hex3d_max_occupants must be in [1, {_abi.GC_SURFEL_MAX_OCCUPANTS}], got {occ}")
    if base_batch is not None and (int(base_batch.n_feat) != int(cfg.n_feat) or
                                   int(base_batch.n_surfel) != int(cfg.n_surfel)):
        raise ValueError(f"base_batch budgets (n_feat {base_batch.n_feat}, n_surfel {base_batch.n_surfel}) differ "
                         f"from the config's ({cfg.n_feat}, {cfg.n_surfel})")


def extract_lidar_surfels(points, timestamps, weights, config: Optional[SurfelExtractionConfig] = None,
                          base_batch: Optional[MeasurementBatch] = None, chart_id: str = GC_CHART_ID,
                          anchor_id: str = "surfel_extraction", ctx=None, device_out: bool = False
                          ) -> Tuple[MeasurementBatch, CertBundle, ExpectedEffect]:
    """lidar_surfel_extraction.py:339-431. points (N, 3), timestamps (N), weights (N): host arrays or
    DeviceArrays (what deskew_constant_twist(..., device_out=True) returns). With base_batch (e.g. camera
    splats) its camera slice, its counts and the unused tail of its LiDAR slice are carried over
    unchanged; otherwise the batch is LiDAR-only. With device_out the nine arrays stay in HBM: they are
    the batch's fields and batch.device. The call waits once, for n_lidar_valid (:206)."""
    cfg = config or SurfelExtractionConfig()
    n = _rows(points, 3)
    _validate(n, _rows(timestamps), _rows(weights), cfg, base_batch)
    n_feat, n_surfel = int(cfg.n_feat), int(cfg.n_surfel)
    n_total = n_feat + n_surfel
    n_lobes = GC_VMF_N_LOBES
    if base_batch is not None:
        esh = tuple(base_batch.etas.shape)
        if len(esh) != 3 or esh[0] != n_total or esh[2] != 3:
            raise ValueError(f"base_batch.etas of shape {esh}, expected ({n_total}, n_lobes, 3)")
        n_lobes = int(esh[1])
    ctx = ctx or _abi.default_context()
    dp = _abi.device_input(ctx, points, np.float64, (n, 3))
    dt = _abi.device_input(ctx, timestamps, np.float64, (n,))
    dw = _abi.device_input(ctx, weights, np.float64, (n,))
    names = list(BATCH_ARRAYS)
    shapes = {k: (n_total,) + (shp if k != "etas" else (n_lobes, 3)) for k, (shp, _, _) in BATCH_ARRAYS.items()}
    # the nine arrays and the slot -> cell record as views of one block: one fill, one download
    blk = _abi.alloc_many(ctx, [(shapes[k], BATCH_ARRAYS[k][2]) for k in names] + [((n_surfel,), np.int32)])
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
    _abi.call("gc_extract_lidar_surfels", ctx.handle, n, dp.ptr, dt.ptr, dw.ptr,
              C.byref(_abi.cfg("gc_surfel_cfg", cfg, n_lobes=n_lobes)),
              *[out[k].ptr for k in names], d_cells.ptr, C.byref(nv), ctx=ctx)
    n_use = int(nv.value)
    counts = dict(n_feat=n_feat, n_surfel=n_surfel, n_lidar_valid=n_use,
                  n_camera_valid=int(base_batch.n_camera_valid) if base_batch is not None else 0)
    if device_out:
        batch = MeasurementBatch(**out, **counts, device=dict(out), lidar_slot_cells=d_cells)
    else:
        host = dict(zip(names + ["cells"], _abi.download_many(blk)))
        cells = host.pop("cells")
        host = {k: v.astype(BATCH_ARRAYS[k][1], copy=False) for k, v in host.items()}
        batch = MeasurementBatch(**host, **counts, lidar_slot_cells=cells)
    cert = CertBundle.create_approx(
        chart_id=chart_id, anchor_id=anchor_id,
        triggers=["ma_hex3d_binning", "plane_fit_batched", "wishart_regularization"],
        support=SupportCert(ess_total=float(n_use), support_frac=float(n_use) / float(max(n_surfel, 1))),
        influence=InfluenceCert.identity())
    return batch, cert, ExpectedEffect(objective_name="surfel_extraction", predicted=float(n_use),
                                       realized=float(n_use))
