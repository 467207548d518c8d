"""VisualPoseEvidence (backend/operators/visual_pose_evidence.py:261-436) on the GPU: 22-D pose
evidence from the OT association of scan primitives with a map view — the WLS translation term
(:74-162) and the vMF scatter rotation term (:165-253). The reference calls it once per hypothesis
with the same association (backend/pipeline.py:978-1008); ``visual_pose_evidence_batched`` takes
all H linearisation poses in one call (gc_visual_pose_evidence: one pose-independent collapse of
the N x K gather, then one workgroup per hypothesis)."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .. import _abi
from ..association import DeviceMapView, PrimitiveAssociationResult
from ..belief import BeliefGaussianInfo
from ..certificates import CertBundle, ExpectedEffect, InfluenceCert, SupportCert
from ..constants import D_Z, GC_CHART_ID, GC_EPS_LIFT, GC_EPS_MASS


@dataclass
class VisualPoseEvidenceResult:
    """visual_pose_evidence.py:50-66."""
    L_pose: np.ndarray  # (22, 22)
    h_pose: np.ndarray  # (22,)
    L_trans: np.ndarray  # (3, 3)
    h_trans: np.ndarray  # (3,)
    L_rot: np.ndarray  # (3, 3)
    h_rot: np.ndarray  # (3,)
    total_weighted_cost: float
    n_associations: int
    mean_transported_mass: float  # mean over valid rows of Σ_k π[i, k]; not normalised


def _association_arrays(ctx, association_result: PrimitiveAssociationResult, V: int):
    """(responsibilities, pool indices, row masses) on the device and (N, K). The association's own
    device arrays are used when it carries them; host arrays are range-checked, then uploaded."""
    dev = getattr(association_result, "device", None)
    if dev is not None:
        r, p, m = dev["responsibilities"], dev["candidate_pool_indices"], dev["row_masses"]
        N, K = r.shape
        return (_abi.device_input(ctx, r, np.float64, (N, K)), _abi.device_input(ctx, p, np.int32, (N, K)),
                _abi.device_input(ctx, m, np.float64, (N,)), N, K)
    resp = np.ascontiguousarray(association_result.responsibilities, np.float64)
    if resp.ndim != 2:
        raise ValueError(f"responsibilities must be (N, K), got {resp.shape}")
    N, K = resp.shape
    idx = np.asarray(association_result.candidate_pool_indices)
    if idx.shape != (N, K):
        raise ValueError(f"candidate_pool_indices of shape {idx.shape}, expected {(N, K)}")
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= V):
        raise ValueError(f"candidate_pool_indices outside the view: range [{int(idx.min())}, {int(idx.max())}], "
                         f"view holds {V} entries")
    rowm = np.ascontiguousarray(association_result.row_masses, np.float64).reshape(-1)
    if rowm.shape[0] != N:
        raise ValueError(f"row_masses of length {rowm.shape[0]}, expected {N}")
    d = _abi.upload_many(ctx, (resp, np.ascontiguousarray(idx, np.int32), rowm), [np.float64, np.int32, np.float64])
    return d[0], d[1], d[2], N, K


def visual_pose_evidence_batched(association_result: PrimitiveAssociationResult, measurement_batch,
                                 map_view: DeviceMapView, poses6, eps_lift: float = GC_EPS_LIFT,
                                 eps_mass: float = GC_EPS_MASS, device_out: bool = False):
    """The evidence of H linearisation poses poses6 (H, 6) = [t, rotvec] from one association, one
    call: (L_pose (H, 22, 22), h_pose (H, 22), parts (H, 26), cert_vec). parts rows are
    [L_trans (9) | h_trans (3) | L_rot (9) | h_rot (3) | cost_trans | cost_rot]; cert_vec =
    [n_valid_meas, n_valid_map, Σ row_masses, mean row mass] over the valid measurement rows. Row h is
    bitwise what the single-pose operator returns for pose h. measurement_batch is duck-typed as in
    associate_primitives_ot: Lambdas (N,3,3), thetas (N,3), etas (N,L,3), valid_mask (N).
    poses6 may be a DeviceArray (H, 6) on the view's context (used in place, no upload). With
    device_out=True L_pose and h_pose come back as DeviceArrays with no download (the batched pipeline's
    set_lidar_evidence takes them as they are); parts and cert_vec are host arrays either way."""
    ctx = map_view.ctx
    d_resp, d_idx, d_rowm, N, K = _association_arrays(ctx, association_result, map_view.count)
    if isinstance(poses6, _abi.DeviceArray):
        H = int(np.prod(poses6.shape)) // 6
        P = _abi.device_input(ctx, poses6, np.float64, (H, 6))
    else:
        P = np.ascontiguousarray(poses6, np.float64).reshape(-1, 6)
        H = P.shape[0]
    etas = measurement_batch.etas
    L = int(np.shape(etas)[1])  # (N, L, 3)
    if int(np.prod(np.shape(measurement_batch.valid_mask))) != N:
        raise ValueError(f"measurement batch of {np.shape(measurement_batch.valid_mask)} rows, association of {N}")
    valid = measurement_batch.valid_mask
    if not isinstance(valid, _abi.DeviceArray):
        valid = np.ascontiguousarray(valid).reshape(-1).astype(np.uint8)
    dLam, dth, deta, dval, dP = _abi.upload_many(
        ctx, (_shaped(measurement_batch.Lambdas, (N, 9)), _shaped(measurement_batch.thetas, (N, 3)),
              _shaped(etas, (N, L * 3)), valid, P), [np.float64, np.float64, np.float64, np.uint8, np.float64])
    dL, dh, dp = _abi.alloc_many(ctx, [(H, D_Z, D_Z), (H, D_Z), (H, _abi.GC_VPE_PARTS)])
    cert = np.zeros(_abi.GC_VPE_CERT)
    _abi.call("gc_visual_pose_evidence", ctx.handle, N, K, L, dLam.ptr, dth.ptr, deta.ptr, dval.ptr, d_resp.ptr,
              d_idx.ptr, d_rowm.ptr, C.byref(map_view.struct), H, dP.ptr, float(eps_lift), float(eps_mass), dL.ptr,
              dh.ptr, dp.ptr, cert.ctypes.data, ctx=ctx)
    if H == 0:
        return np.zeros((0, D_Z, D_Z)), np.zeros((0, D_Z)), np.zeros((0, _abi.GC_VPE_PARTS)), cert
    if device_out:
        return dL, dh, dp.download(), cert
    Lp, hp, parts = _abi.download_many([dL, dh, dp])
    return Lp, hp, parts, cert


def _shaped(x, shape):
    return x if isinstance(x, _abi.DeviceArray) else np.ascontiguousarray(x, np.float64).reshape(shape)


def visual_pose_evidence(association_result: PrimitiveAssociationResult, measurement_batch, map_view: DeviceMapView,
                         belief_pred: Optional[BeliefGaussianInfo], eps_lift: float = GC_EPS_LIFT,
                         eps_mass: float = GC_EPS_MASS, chart_id: str = GC_CHART_ID,
                         anchor_id: str = "visual_pose_evidence", z_lin_pose=None
                         ) -> Tuple[VisualPoseEvidenceResult, CertBundle, ExpectedEffect]:
    """visual_pose_evidence.py:261-436. The linearisation pose is z_lin_pose ([t, rotvec]) when given,
    else belief_pred.world_pose(eps_lift)."""
    if z_lin_pose is not None:
        pose = np.asarray(z_lin_pose, np.float64).ravel()[:6]
    else:
        pose = belief_pred.world_pose(eps_lift, ctx=map_view.ctx)[:6]
    Lp, hp, parts, cv = visual_pose_evidence_batched(association_result, measurement_batch, map_view, pose[None],
                                                     eps_lift, eps_mass)
    p = parts[0]
    n_valid, n_map, K = int(cv[0]), int(cv[1]), int(np.shape(association_result.responsibilities)[1])
    empty = n_valid == 0 or n_map == 0
    cost = float(p[24] + p[25])
    result = VisualPoseEvidenceResult(
        L_pose=Lp[0], h_pose=hp[0], L_trans=p[0:9].reshape(3, 3).copy(), h_trans=p[9:12].copy(),
        L_rot=p[12:21].reshape(3, 3).copy(), h_rot=p[21:24].copy(), total_weighted_cost=cost,
        n_associations=0 if empty else n_valid * K, mean_transported_mass=0.0 if empty else float(cv[3]))
    if empty:  # :297-318
        return (result, CertBundle.create_exact(chart_id=chart_id, anchor_id=anchor_id),
                ExpectedEffect(objective_name="visual_pose_evidence", predicted=0.0, realized=0.0))
    cert = CertBundle.create_approx(
        chart_id=chart_id, anchor_id=anchor_id, triggers=["linearization", "ot_soft_correspondence"],
        frobenius_applied=True, support=SupportCert(ess_total=float(cv[2]), support_frac=1.0),
        influence=InfluenceCert.identity().with_overrides(lift_strength=eps_lift))
    return result, cert, ExpectedEffect(objective_name="visual_pose_evidence", predicted=cost, realized=cost)


def build_visual_pose_evidence_22d(visual_result: VisualPoseEvidenceResult) -> Tuple[np.ndarray, np.ndarray]:
    """visual_pose_evidence.py:444-454: the (22, 22) precision and (22,) information vector for the fusion."""
    return visual_result.L_pose, visual_result.h_pose
