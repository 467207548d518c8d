"""MeasurementBatch (backend/structures/measurement_batch.py:68-157): the fixed-size batch of
measurement primitives the OT association and VisualPoseEvidence consume. Camera splats occupy rows
[0, n_feat), LiDAR surfels rows [n_feat, n_feat + n_surfel); geometry in information form
(Lambdas, thetas), orientation as multi-lobe vMF natural parameters (etas).

``device`` follows PrimitiveAssociationResult.device: when an operator computed the batch on the GPU
(ops.extract_lidar_surfels) it holds the same nine arrays as the DeviceArrays they were computed
into, and a consumer on the device reads them in HBM instead of uploading the host copies."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from .constants import GC_N_FEAT, GC_N_SURFEL, GC_VMF_N_LOBES

# the nine batch arrays: name -> (trailing shape, host dtype, device dtype)
BATCH_ARRAYS = dict(Lambdas=((3, 3), np.float64, np.float64), thetas=((3,), np.float64, np.float64),
                    etas=((GC_VMF_N_LOBES, 3), np.float64, np.float64), weights=((), np.float64, np.float64),
                    sources=((), np.int32, np.int32), source_indices=((), np.int32, np.int32),
                    valid_mask=((), np.bool_, np.uint8), timestamps=((), np.float64, np.float64),
                    colors=((3,), np.float64, np.float64))


@dataclass
class MeasurementBatch:
    """measurement_batch.py:68-134. With device_out the nine array fields are DeviceArrays (the same
    objects as in ``device``); otherwise host arrays. ``lidar_slot_cells`` (n_surfel, int32; -1 past
    n_lidar_valid) is a diagnostic of the device extraction: the hash cell each LiDAR slot came from;
    ``depth_slot_cells`` (n_feat, int32) likewise the image cell of every camera row that
    ops.extract_depth_surfels wrote, -1 for the rows it did not."""
    Lambdas: np.ndarray         # (n_total, 3, 3)
    thetas: np.ndarray          # (n_total, 3)
    etas: np.ndarray            # (n_total, GC_VMF_N_LOBES, 3)
    weights: np.ndarray         # (n_total,)
    sources: np.ndarray         # (n_total,) int32: 0 = camera, 1 = lidar
    source_indices: np.ndarray  # (n_total,) int32
    valid_mask: np.ndarray      # (n_total,) bool
    timestamps: np.ndarray      # (n_total,)
    colors: np.ndarray          # (n_total, 3)
    n_feat: int
    n_surfel: int
    n_camera_valid: int
    n_lidar_valid: int
    device: Optional[dict] = None
    lidar_slot_cells: Optional[np.ndarray] = None
    depth_slot_cells: Optional[np.ndarray] = None

    @property
    def n_total(self) -> int:
        return self.n_feat + self.n_surfel

    @property
    def n_valid(self) -> int:
        return self.n_camera_valid + self.n_lidar_valid

    @property
    def camera_slice(self) -> slice:
        return slice(0, self.n_feat)

    @property
    def lidar_slice(self) -> slice:
        return slice(self.n_feat, self.n_total)


def create_empty_measurement_batch(n_feat: int = GC_N_FEAT, n_surfel: int = GC_N_SURFEL) -> MeasurementBatch:
    """measurement_batch.py:137-157."""
    n_total = int(n_feat) + int(n_surfel)
    arrays = {k: np.zeros((n_total,) + shp, dt) for k, (shp, dt, _) in BATCH_ARRAYS.items()}
    return MeasurementBatch(**arrays, n_feat=int(n_feat), n_surfel=int(n_surfel), n_camera_valid=0, n_lidar_valid=0)
