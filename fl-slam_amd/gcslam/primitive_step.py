"""The reference's current scan step (backend/pipeline.py:778-1327) on the device, end to end: the
batched pipeline in GC_LIDAR_GIVEN mode around the primitive-map branch,

    pipeline front (predict, IMU/odom branch, z_lin_pose)            pipeline.py:400-776
      -> deskew with hypothesis 0's twist, surfel extraction         :520-560, :781-800
      -> MapBranch.front (tiles, recency inflate, OT association,
         visual_pose_evidence at every hypothesis's z_lin_pose)      :802-1015
      -> pipeline back (evidence sum, tempering, fusion, recompose)  :1038-1230
      -> exchange / combine / IW apply                               backend_node.py:2036-2119
      -> MapBranch.update at z_t                                     :1232-1492

with the linearisation poses and the evidence staying in HBM between the steps.

Semantics for H > 1 hypotheses (MapBranch's design: one measurement batch and one association per
scan): the batch is built from the scan deskewed with global hypothesis 0's twist, every hypothesis
gets its own linearisation pose and so its own evidence, and the map is updated at hypothesis 0's
z_t. At H = 1 this is the reference step. Single rank only: a rank without hypothesis 0 has no twist
to deskew with."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional, Sequence, Tuple

import numpy as np

from .certificates import CertBundle, InfluenceCert, SupportCert, aggregate_certificates
from .constants import GC_CHART_ID
from .map_branch import MapBranch, MapBranchFront
from .ops.depth_pose_evidence import MAX_POSES, DepthEvidenceConfig, depth_pose_evidence_batched
from .ops.depth_pose_evidence import result_from_parts as depth_result
from .ops.photometric_pose_evidence import PhotometricEvidenceConfig, rgbd_pose_evidence_batched
from .ops.photometric_pose_evidence import result_from_parts as photo_result
from .ops.deskew_constant_twist import deskew_constant_twist
from .ops.depth_surfel_extraction import DepthSurfelConfig, extract_depth_surfels
from .ops.lidar_surfel_extraction import SurfelExtractionConfig, extract_lidar_surfels
from .ops.point_budget import point_budget_resample
from .pipeline import BatchedScanPipeline


def lidar_cert_row(evidence_certs: Sequence[CertBundle], extra_trigger_certs: Sequence[CertBundle] = ()) -> np.ndarray:
    """The GC_LIDAR_CERT row of gc_pipeline_set_lidar_evidence: [ess_total, support_frac, nll_per_ess,
    exc_dt, exc_ex] of aggregate_certificates(evidence_certs) = [deskew, surfel, assoc, visual]
    (pipeline.py:1056-1064), then the summed trigger magnitudes of evidence_certs and
    extra_trigger_certs (the recency inflation's certificate is in all_certs, :1211, but not among
    the LiDAR evidence certificates)."""
    agg = aggregate_certificates(list(evidence_certs))
    trig = 0.0
    for c in list(evidence_certs) + list(extra_trigger_certs):
        trig = trig + float(c.total_trigger_magnitude())
    return np.array([agg.support.ess_total, agg.support.support_frac, agg.mismatch.nll_per_ess,
                     agg.excitation.dt_effect, agg.excitation.extrinsic_effect, trig], np.float64)


def visual_cert(vpe_cert: np.ndarray, eps_lift: float, chart_id: str = GC_CHART_ID) -> CertBundle:
    """visual_pose_evidence's certificate (visual_pose_evidence.py:297-318, :420-436) from the batched
    operator's cert_vec [n_valid_meas, n_valid_map, sum row_masses, mean row mass]: the same for every
    hypothesis (it does not depend on the pose)."""
    if int(vpe_cert[0]) == 0 or int(vpe_cert[1]) == 0:
        return CertBundle.create_exact(chart_id=chart_id, anchor_id="visual_pose_evidence")
    return CertBundle.create_approx(
        chart_id=chart_id, anchor_id="visual_pose_evidence", triggers=["linearization", "ot_soft_correspondence"],
        frobenius_applied=True, support=SupportCert(ess_total=float(vpe_cert[2]), support_frac=1.0),
        influence=InfluenceCert.identity().with_overrides(lift_strength=float(eps_lift)))


@dataclass
class PrimitiveStepResult:
    front: MapBranchFront
    update: Tuple[Any, CertBundle, Any]  # MapBranch.update's (result, cert, effect)
    combined: dict                       # BatchedScanPipeline.combined()
    lidar_cert: np.ndarray               # the GC_LIDAR_CERT row the back ran on
    z_t: np.ndarray                      # hypothesis 0's recomposed world pose, the update's pose
    xi_body: np.ndarray                  # hypothesis 0's deskew twist
    certs: list                          # [deskew, surfel(, depth surfels), recency inflate, assoc, visual(, depth(, photometric))]
    depth_parts: Optional[np.ndarray] = None  # with a depth frame: the (H, GC_DEPTHEV_PARTS) rows that were added
    photo_parts: Optional[np.ndarray] = None  # with rgb or luminance in the frame: the luminance rows, likewise


class PrimitiveScanStep:
    def __init__(self, pipeline: BatchedScanPipeline, map_branch: MapBranch,
                 surfel_config: Optional[SurfelExtractionConfig] = None):
        if pipeline.world != 1:
            raise ValueError("PrimitiveScanStep is single rank: a rank without hypothesis 0 has no twist to "
                             f"deskew with (world_size = {pipeline.world})")
        if pipeline.ctx is not map_branch.atlas_map.ctx:
            raise ValueError("the pipeline and the map must share one context (the evidence is handed over "
                             "on its stream)")
        self.pipeline, self.branch = pipeline, map_branch
        self.surfel_config = surfel_config or SurfelExtractionConfig()
        pipeline.set_lidar_mode(True)

    def measurement_batch(self, scan: dict, xi_body, ess_imu: float):
        """pipeline.py:500-560, :781-800: budget -> deskew with xi_body -> surfels, on the device.
        Returns (batch, deskew cert, surfel cert)."""
        ctx, chart = self.pipeline.ctx, self.branch.chart_id
        bud, _, _ = point_budget_resample(scan["points"], scan["timestamps"], scan["weights"],
                                          n_points_cap=self.pipeline.cfg.n_points_cap, chart_id=chart, ctx=ctx,
                                          device_out=True)
        dsk, dsk_cert, _ = deskew_constant_twist(bud.points, bud.timestamps, bud.weights, float(scan["scan_start"]),
                                                 float(scan["scan_end"]), xi_body, float(ess_imu), chart,
                                                 "deskew_constant_twist", ctx=ctx, device_out=True)
        batch, surfel_cert, _ = extract_lidar_surfels(dsk.points, dsk.timestamps, dsk.weights, self.surfel_config,
                                                      chart_id=chart, ctx=ctx, device_out=True)
        return batch, dsk_cert, surfel_cert

    def depth_surfels(self, batch, depth_frame: dict, timestamp: float):
        """The camera slice of the scan's batch filled from the RGB-D frame (ops/depth_surfel_extraction.py),
        after the camera rows the batch already holds. Returns (batch, depth surfel cert)."""
        cfg = depth_frame["surfels"]
        if not isinstance(cfg, DepthSurfelConfig):
            cfg = DepthSurfelConfig(n_feat=int(batch.n_feat), n_surfel=int(batch.n_surfel))
        batch, cert, _ = extract_depth_surfels(
            depth_frame["depth"], depth_frame.get("rgb"), depth_frame["intrinsics"], depth_frame.get("R_base_camera"),
            depth_frame.get("t_base_camera"), float(depth_frame.get("timestamp", timestamp)), cfg, base_batch=batch,
            chart_id=self.branch.chart_id, ctx=self.pipeline.ctx, device_out=True)
        return batch, cert

    def run(self, slot: int, scan: dict, scan_count: int, timestamp: float, measurement_batch=None,
            batch_certs: Sequence[CertBundle] = (), depth_frame: Optional[dict] = None) -> PrimitiveStepResult:
        """One scan. With measurement_batch the caller's batch is used (batch_certs: its deskew / surfel
        certificates, if any); otherwise it is built from the scan deskewed with hypothesis 0's twist.

        depth_frame (an RGB-D depth frame of this scan): a dict with `depth` (H, W; float32 metres, host or
        device) and `intrinsics` (PinholeIntrinsics), and optionally `R_base_camera`, `t_base_camera`,
        `view_cfg` (CameraViewConfig) and `cfg` (DepthEvidenceConfig). The depth pose evidence
        (ops/depth_pose_evidence.py) of every hypothesis's linearisation pose against the map as it
        stands after MapBranch.front is added on the device into the front's L_lidar / h_lidar, and
        hypothesis 0's certificate joins the evidence certificates. At most 32 hypotheses.

        The frame may also carry `rgb` ((H, W, 3) uint8) or `luminance` ((H, W) float, NaN for a hole) of the
        same camera, and `photo_cfg` (PhotometricEvidenceConfig): then the depth and the photometric
        evidence (ops/photometric_pose_evidence.py: rgbd_pose_evidence_batched) are added, in that order,
        and hypothesis 0's photometric certificate follows the depth one. `depth` stays required.

        With `surfels` (True, or a DepthSurfelConfig whose budgets are the batch's) the frame also feeds the
        map: once the scan's batch is there (built or the caller's) and before MapBranch.front, the free rows
        of its camera slice are filled with the coloured surfels of `depth` and `rgb`
        (ops/depth_surfel_extraction.py; a `luminance`-only frame gives rows without colour), at the frame's
        extrinsics and its `timestamp` (default: the scan's). Their certificate follows the surfel one in
        batch_certs, so it is in the GC_LIDAR_CERT aggregate and in `certs`. Without the key nothing of the
        step changes."""
        pipe, br = self.pipeline, self.branch
        if depth_frame is not None:
            if pipe.Hl > MAX_POSES:
                raise ValueError(f"{pipe.Hl} hypotheses with a depth frame; at most {MAX_POSES} are supported")
            if "depth" not in depth_frame or "intrinsics" not in depth_frame:
                raise ValueError("depth_frame needs `depth` and `intrinsics`")
            if depth_frame.get("rgb") is not None and depth_frame.get("luminance") is not None:
                raise ValueError("depth_frame carries `rgb` or `luminance`, not both")
        pipe.stage_scan(slot, scan)
        pipe.scan_front(slot, scan, scan_count)
        # the one small download before the map branch (the reference's own sync, pipeline.py:811):
        # hypothesis 0's deskew twist and predicted position (the map centre)
        xi0, ess0, pose_pred0 = pipe.front_hyp0()
        lin_d, _ = pipe.front_poses(device=True)
        center = pose_pred0[0:3].copy()
        if measurement_batch is None:
            measurement_batch, dsk_cert, surfel_cert = self.measurement_batch(scan, xi0, ess0)
            batch_certs = [dsk_cert, surfel_cert]
        if depth_frame is not None and depth_frame.get("surfels"):
            measurement_batch, ds_cert = self.depth_surfels(measurement_batch, depth_frame, timestamp)
            batch_certs = list(batch_certs) + [ds_cert]
        front = br.front(measurement_batch, center, lin_d, int(scan_count), device_out=True)
        inflate_cert, assoc_cert = front.certs
        vcert = visual_cert(front.vpe_cert, br.config.eps_lift, br.chart_id)
        evidence_certs = list(batch_certs) + [assoc_cert, vcert]
        depth_certs, depth_parts, photo_parts = [], None, None
        if depth_frame is not None:
            dcfg, pcfg = depth_frame.get("cfg") or DepthEvidenceConfig(), None
            image = depth_frame.get("rgb") if depth_frame.get("rgb") is not None else depth_frame.get("luminance")
            where = (br.atlas_map, depth_frame["intrinsics"], lin_d)
            camera = (depth_frame.get("R_base_camera"), depth_frame.get("t_base_camera"), depth_frame.get("view_cfg"))
            into = (front.device["L_lidar"], front.device["h_lidar"])
            if image is None:
                _, _, parts, render = depth_pose_evidence_batched(*where, depth_frame["depth"], *camera, dcfg,
                                                                  accumulate_into=into, device_out=True)
                depth_parts = parts
            else:
                pcfg = depth_frame.get("photo_cfg") or PhotometricEvidenceConfig(eps_lift=dcfg.eps_lift)
                _, _, parts, render = rgbd_pose_evidence_batched(*where, depth_frame["depth"], image, *camera, dcfg,
                                                                        pcfg, accumulate_into=into, device_out=True)
                depth_parts, photo_parts = np.ascontiguousarray(parts[:, 0]), np.ascontiguousarray(parts[:, 1])
            shape = render["depth"].shape[1:]
            for read, rows, cfg in ((depth_result, depth_parts, dcfg), (photo_result, photo_parts, pcfg)):
                if rows is not None:  # hypothesis 0's certificate
                    depth_certs.append(read(None, None, rows[0], shape, cfg.eps_lift, br.chart_id)[1])
        row = lidar_cert_row(evidence_certs + depth_certs, [inflate_cert])
        pipe.set_lidar_evidence(front.device["L_lidar"], front.device["h_lidar"], row)
        pipe.scan_back()
        pipe.finish_scan()
        z_t = pipe.scan_map_pose()[0].copy()
        upd = br.update(front, z_t, float(timestamp))
        return PrimitiveStepResult(front=front, update=upd, combined=pipe.combined(), lidar_cert=row, z_t=z_t,
                                   xi_body=xi0.copy(),
                                   certs=list(batch_certs) + [inflate_cert, assoc_cert, vcert] + depth_certs,
                                   depth_parts=depth_parts, photo_parts=photo_parts)
