"""The map branch of one scan as one object: the reference's _compute_map_branch
(backend/pipeline.py:802-926) from the tile stencils on, its visual_pose_evidence call (:998-1010)
batched over the hypotheses, and the post-pose map update (step 12b, :1232-1492), chained over the
device operators of this package in the reference's order, on a map that follows the robot
(DevicePrimitiveMap.ensure_tiles).

    branch = MapBranch(device_map, MapBranchConfig())
    front = branch.front(measurement_batch, center_xyz, poses6, scan_seq)   # L_lidar, h_lidar, ...
    ...                                                                     # fuse the evidence, pick z_t
    result, cert, effect = branch.update(front, pose_world, timestamp)

Arrays stay in HBM between the steps wherever the operators accept `.device` arrays (the batch of
ops.extract_lidar_surfels, the association result, the view); the recency inflate and the candidate
statistics are launched back to back and read with one download."""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from . import _abi
from .association import (CANDIDATE_STATS, GC_K_ASSOC, GC_K_SINKHORN, GC_M_TILE_VIEW, GC_R_STENCIL_TILES_XY,
                          GC_R_STENCIL_TILES_Z, AssociationConfig, DeviceMapView, PrimitiveAssociationResult,
                          _candidate_stats_launch, associate_primitives_ot, extract_atlas_map_view)
from .certificates import CertBundle, ExpectedEffect
from .constants import (GC_CHART_ID, GC_EPS_LIFT, GC_EPS_MASS, GC_H_TILE, GC_RECENCY_DECAY_LAMBDA,
                        GC_RECENCY_MIN_SCALE)
from .ops.visual_pose_evidence import visual_pose_evidence_batched
from .primitive_map import (DevicePrimitiveMap, MapUpdateConfig, PrimitiveMapRecencyInflateStats,
                            PrimitiveMapUpdateResult, TileResidency, _recency_tiles_dense, _recency_tiles_finish,
                            _recency_tiles_launch, primitive_map_update_from_association)
from .tiling import ma_hex_stencil_tile_ids

GC_R_ACTIVE_TILES_XY = 1  # constants.py:411
GC_R_ACTIVE_TILES_Z = 0   # constants.py:412


def _stencil_count(radius_xy: int, radius_z: int) -> int:
    """constants.py:419-433: a hex disk times a symmetric slab."""
    return (2 * int(radius_z) + 1) * (3 * int(radius_xy) * (int(radius_xy) + 1) + 1)


@dataclass
class MapBranchConfig:
    """The PipelineConfig fields the map branch reads (pipeline.py:96-207), under the reference's names."""
    H_TILE: float = GC_H_TILE
    N_ACTIVE_TILES: int = _stencil_count(GC_R_ACTIVE_TILES_XY, GC_R_ACTIVE_TILES_Z)
    R_ACTIVE_TILES_XY: int = GC_R_ACTIVE_TILES_XY
    R_ACTIVE_TILES_Z: int = GC_R_ACTIVE_TILES_Z
    M_TILE_VIEW: int = GC_M_TILE_VIEW
    N_STENCIL_TILES: int = _stencil_count(GC_R_STENCIL_TILES_XY, GC_R_STENCIL_TILES_Z)
    R_STENCIL_TILES_XY: int = GC_R_STENCIL_TILES_XY
    R_STENCIL_TILES_Z: int = GC_R_STENCIL_TILES_Z
    k_assoc: int = GC_K_ASSOC
    k_sinkhorn: int = GC_K_SINKHORN
    ot_epsilon: float = 0.1
    ot_tau_a: float = 0.5
    ot_tau_b: float = 0.5
    RECENCY_DECAY_LAMBDA: float = GC_RECENCY_DECAY_LAMBDA
    RECENCY_MIN_SCALE: float = GC_RECENCY_MIN_SCALE
    eps_lift: float = GC_EPS_LIFT
    eps_mass: float = GC_EPS_MASS
    map_update: MapUpdateConfig = field(default_factory=MapUpdateConfig)

    def association_config(self, scan_seq: int) -> AssociationConfig:
        """pipeline.py:854-866."""
        return AssociationConfig(k_assoc=self.k_assoc, k_sinkhorn=self.k_sinkhorn, epsilon=self.ot_epsilon,
                                 tau_a=self.ot_tau_a, tau_b=self.ot_tau_b, eps_mass=self.eps_mass,
                                 h_tile=float(self.H_TILE), r_stencil_tiles_xy=int(self.R_STENCIL_TILES_XY),
                                 r_stencil_tiles_z=int(self.R_STENCIL_TILES_Z), scan_seq=int(scan_seq),
                                 recency_decay_lambda=float(self.RECENCY_DECAY_LAMBDA))


@dataclass
class MapBranchFront:
    """What the branch computes before the pose is known (the dict of pipeline.py:909-926 and the
    evidence of :998-1010 for every hypothesis)."""
    L_lidar: np.ndarray   # (H, 22, 22)
    h_lidar: np.ndarray   # (H, 22)
    vpe_parts: np.ndarray  # (H, GC_VPE_PARTS)
    vpe_cert: np.ndarray   # GC_VPE_CERT values
    assoc_result: PrimitiveAssociationResult
    map_view: DeviceMapView
    measurement_batch: Any
    active_tile_ids: List[int]
    stencil_tile_ids: List[int]
    certs: List[CertBundle]          # recency inflate, association
    inflate_stats: PrimitiveMapRecencyInflateStats
    residency: TileResidency
    map_branch_stats: Dict[str, float]  # the six floats of pipeline.py:920-925
    scan_seq: int
    device: Optional[Dict[str, Any]] = None  # with device_out: L_lidar / h_lidar as DeviceArrays (no download)


class MapBranch:
    """The per-scan map branch on one DevicePrimitiveMap. `front` makes the scan's tiles resident and
    computes the pose evidence of every hypothesis from one association; `update` is step 12b at the
    chosen pose with the maintenance on the device."""

    def __init__(self, atlas_map: DevicePrimitiveMap, config: Optional[MapBranchConfig] = None,
                 chart_id: str = GC_CHART_ID):
        self.atlas_map = atlas_map
        self.config = config or MapBranchConfig()
        self.chart_id = chart_id

    def front(self, measurement_batch, center_xyz, poses6, scan_seq: int, device_out: bool = False
              ) -> MapBranchFront:
        """poses6 (H, 6): host array or DeviceArray. device_out=True keeps L_lidar / h_lidar on the device:
        the front's L_lidar / h_lidar are then DeviceArrays (np.asarray downloads them), also under
        `.device`."""
        cfg, dm = self.config, self.atlas_map
        ctx = dm.ctx
        center = np.asarray(center_xyz, np.float64).reshape(3)
        active = ma_hex_stencil_tile_ids(center, float(cfg.H_TILE), int(cfg.R_ACTIVE_TILES_XY),
                                         int(cfg.R_ACTIVE_TILES_Z))
        stencil = ma_hex_stencil_tile_ids(center, float(cfg.H_TILE), int(cfg.R_STENCIL_TILES_XY),
                                          int(cfg.R_STENCIL_TILES_Z))
        if len(active) != int(cfg.N_ACTIVE_TILES):
            raise ValueError(f"active tile stencil size mismatch: expected N_ACTIVE_TILES={cfg.N_ACTIVE_TILES}, "
                             f"got {len(active)}")
        if len(stencil) != int(cfg.N_STENCIL_TILES):
            raise ValueError(f"stencil tile size mismatch: expected N_STENCIL_TILES={cfg.N_STENCIL_TILES}, "
                             f"got {len(stencil)}")
        residency = dm.ensure_tiles(list(dict.fromkeys(active + stencil)))  # active ∪ stencil, in order

        # the recency inflate of the active tiles (pipeline.py:835-843), launched with no wait; its
        # statistics come down with the candidate statistics below
        dense = _recency_tiles_dense(dm, active)
        h_dense = np.asarray(dense, np.int32)
        d_dense, = _abi.upload_many(ctx, [h_dense], [np.int32])
        d_inflate, d_cand = _abi.alloc_many(ctx, [((max(len(dense), 1), 3), np.float64), ((3,), np.float64)])
        _recency_tiles_launch(dm, d_dense, h_dense, scan_seq, cfg.RECENCY_DECAY_LAMBDA, cfg.RECENCY_MIN_SCALE,
                              d_inflate)

        view = extract_atlas_map_view(dm, stencil, int(cfg.M_TILE_VIEW), cfg.eps_lift, cfg.eps_mass)
        assoc, assoc_cert, _ = associate_primitives_ot(measurement_batch, view, cfg.association_config(scan_seq),
                                                       chart_id=self.chart_id, anchor_id="primitive_ot")
        _candidate_stats_launch(assoc, measurement_batch, view, cfg.eps_mass, d_cand)
        h_inflate, h_cand = _abi.download_many([d_inflate, d_cand])  # the one download of the two
        _, inflate_cert, _, inflate_stats = _recency_tiles_finish(dm, h_inflate[:len(dense)], self.chart_id,
                                                                  "primitive_map_recency_inflate")

        L_lidar, h_lidar, parts, vpe_cert = visual_pose_evidence_batched(assoc, measurement_batch, view, poses6,
                                                                        cfg.eps_lift, cfg.eps_mass,
                                                                        device_out=device_out)
        stats = dict(zip(CANDIDATE_STATS, (float(v) for v in h_cand)))
        stats.update(staleness_inflation_strength=float(inflate_stats.staleness_inflation_strength),
                     staleness_cov_inflation_trace=float(inflate_stats.staleness_cov_inflation_trace),
                     stale_precision_downscale_total=float(inflate_stats.stale_precision_downscale_total))
        return MapBranchFront(L_lidar=L_lidar, h_lidar=h_lidar, vpe_parts=parts, vpe_cert=vpe_cert, assoc_result=assoc,
                              map_view=view, measurement_batch=measurement_batch, active_tile_ids=active,
                              stencil_tile_ids=stencil, certs=[inflate_cert, assoc_cert],
                              inflate_stats=inflate_stats, residency=residency, map_branch_stats=stats,
                              scan_seq=int(scan_seq),
                              device=dict(L_lidar=L_lidar, h_lidar=h_lidar) if device_out else None)

    def update(self, front: MapBranchFront, pose_world, timestamp: float
               ) -> Tuple[PrimitiveMapUpdateResult, CertBundle, ExpectedEffect]:
        """Step 12b (pipeline.py:1232-1492) at z_t = pose_world = [t, rotvec] with the scan's association,
        cull / forget / merge-reduce on the device behind it: one pass, one wait."""
        return primitive_map_update_from_association(
            self.atlas_map, front.assoc_result, front.measurement_batch, front.active_tile_ids, pose_world,
            float(timestamp), front.scan_seq, self.config.map_update, map_branch_stats=front.map_branch_stats,
            maintenance="device", chart_id=self.chart_id)
