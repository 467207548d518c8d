"""TEST INFRASTRUCTURE — records what the ten operators that take a configuration computed while that
configuration travelled as a bare double vector unpacked by position, for the bit-identity check of
tests/test_gpu_cfg_parent_bits.py. Run on an MI355X with the library built from the commit BEFORE the
configuration became header structs (3b6486e):

    python tests/golden/make_cfg_parent.py

  cfg_parent.npz   "in/<operator>/<array>" the inputs, "out/<operator>/<array>" what the library returned.

Written against the public Python API only, so the same file runs before and after the change. Every
operator is called once, on its smallest shape, with a configuration in which every field the operator
reads differs from its default and from every other field of the same configuration as far as the field's
domain allows, flags and enumerations at a non-default member: reading one field where the neighbouring one
was meant then changes the output. cov_reg_eps and lidar_incidence_sigma_scale, which nothing reads, keep
their defaults. The values that coincide inside one struct are the ones the domain or the case shape forces:
the 4 x 4 surfel grid; in gc_camfeat_cfg the mode code 3 with hex_radius 3 and the model code 1 with
quad_fit_radius 1 (both radii have only 1 and 3 beside their default 2); in gc_ot_cfg r_stencil_tiles_z = 1 with
the flag weight_proportional = 1 (r_z = 2 would equal r_xy = 2, and r_xy = 3 with it exceeds the 128-tile stencil).

    pipeline   BatchedScanPipeline: H = 2, 256 points, one scan with the IMU/odom branch computed: the
               combined record, the beliefs, the IW state and the bin map after it.
    mapupdate  primitive_map_update_from_association on 2 tiles of 32 slots, 32 rows with K = 4 candidates.
    maintain   primitive_map_maintain on 2 tiles of 32 slots.
    ot         associate_primitives_ot: 32 rows against a view of 2 tiles of 16 slots.
    surfel     extract_lidar_surfels: 512 points on a 4 x 4 x 2 grid.
    cam        camera_measurement_batch(return_diag=True): 256 points, 8 features (the depth evidence of
               lidar_depth_evidence is its first step and comes back in the diagnostics).
    camfeat    lift_camera_features: a 48 x 64 depth image, 16 keypoints.
    kp         detect_keypoints(return_pyramid=True): a 64 x 48 image, 2 levels (keypoints_plan inside).
    bev        bev_splat_prep and render_ewa_tiles: 32 primitives, one 32 x 32 view, tile 16, cap 4.
    camview    camera_splat_prep and render_depth_tiles: the same.

The inputs are drawn here from fixed seeds and stored with the outputs; the test reads them from the file
and never rebuilds them, so it does not depend on how the host evaluates sin, exp or a matrix product.
Arrays are compared as bytes: NaN and inf entries (a query without LiDAR evidence, the depth of an invalid
splat) are part of the record. `python tests/golden/make_cfg_parent.py --twice` runs every operator a second
time on the same inputs and reports which outputs differ (none did at 3b6486e, the OT association and the
pipeline, whose order of summation the header does not state, included).
"""

from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (TESTS, os.path.join(ROOT, "fl-slam_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "cfg_parent.npz")
L = 3  # GC_VMF_N_LOBES


class _Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _spd(rng, n, scale, ridge):
    B = rng.normal(size=(n, 3, 3)) * scale
    return np.einsum("nij,nkj->nik", B, B) + ridge * np.eye(3)


# --------------------------------------------------------------------------------------------- pipeline
PIPE_H, PIPE_N_AZ = 2, 16  # 16 rings x 16 azimuth steps = 256 points
PIPE_CFG = dict(tau=0.12, lidar_origin=(-0.05, -0.11, 0.13), eps_psd=2e-12, eps_lift=3e-9, eps_mass=4e-12,
                lambda_ou=0.15, c_frob=0.9, forgetting_factor=0.97, weight_floor=0.004, power_beta_min=0.3,
                power_beta_exc_c=40.0, power_beta_z_c=1.3, alpha_min=0.8, alpha_max=0.95, c0_cond=2e6, nu_max=800.0,
                planar_z_ref=0.07, planar_z_sigma=0.2, planar_vz_sigma=0.02, imu_gravity_scale=1.05)


def in_pipeline():
    from oracle import cases
    case = cases.build(H=PIPE_H, n_az=PIPE_N_AZ, n_scans=1, io="computed")
    out = {"scan_" + k: np.asarray(v) for k, v in case["scans"][0].items()}
    out.update({"hyp_" + k: np.asarray(v) for k, v in case["hyp"].items()})
    out.update({f"iw_{i}": np.asarray(v) for i, v in enumerate(case["iw"])})
    out["map_record"] = case["map_record"]
    return out


def run_pipeline(ctx, inp):
    from gcslam.pipeline import BatchedScanPipeline, PipelineConfig
    s = {k[5:]: (v if v.ndim else v.item()) for k, v in inp.items() if k.startswith("scan_")}
    hy = {k[4:]: v for k, v in inp.items() if k.startswith("hyp_")}
    n = s["points"].shape[0]
    pipe = BatchedScanPipeline(PIPE_H, n, PipelineConfig(n_points_cap=n, **PIPE_CFG), ctx=ctx)
    pipe.set_beliefs(hy["X_anchor"], hy["z_lin"], hy["L"], hy["h"], hy["stamp"])
    pipe.set_weights(hy["weights"])
    pipe.set_io_mode(True)
    pipe.set_iw(*[inp[f"iw_{i}"] for i in range(4)])
    pipe.set_map(inp["map_record"])
    pipe.stage_scan(0, s)
    pipe.run_scan(0, s, 0)
    ctx.sync()
    c = pipe.combined()
    out = {"combined_" + k: np.asarray(v) for k, v in c.items()}
    out.update({"belief_" + k: v for k, v in pipe.get_beliefs().items()})
    out.update({"iw_" + k: np.asarray(v) for k, v in pipe.get_iw().items()})
    out["map"] = pipe.get_map()["map"]
    out["hyp_diag"] = pipe.hyp_diag()
    pipe.close()
    return out


# --------------------------------------------------------------------------------------------- the map
MAP_M = 32
MAP_CELLS = ((0, 0, 0), (3, 0, 0))


def _map_fields(rng, n_tiles, m_tile, h):
    """Flat (n_tiles * m_tile, ...) map fields, tile d inside the cell MAP_CELLS[d] of tiles of width h."""
    M = n_tiles * m_tile
    pos = np.zeros((M, 3))
    for d, (c1, c2, cz) in enumerate(MAP_CELLS[:n_tiles]):
        s1 = rng.uniform(c1 * h, (c1 + 1) * h, m_tile)
        s2 = rng.uniform(c2 * h, (c2 + 1) * h, m_tile)
        pos[d * m_tile:(d + 1) * m_tile] = np.column_stack([s1, (s2 - 0.5 * s1) / (np.sqrt(3.0) * 0.5),
                                                            rng.uniform(cz * h, (cz + 1) * h, m_tile)])
    Lam = _spd(rng, M, 0.3, 2.0)
    f = dict(Lambdas=Lam, thetas=np.einsum("nij,nj->ni", Lam, pos), etas=rng.normal(size=(M, L, 3)) * 2.0,
             weights=rng.uniform(0.0, 1.0, M) ** 3, timestamps=rng.uniform(0.0, 5.0, M),
             created_timestamps=rng.uniform(0.0, 5.0, M),
             last_supported_scan_seq=rng.integers(0, 12, M).astype(np.int64),
             last_update_scan_seq=rng.integers(0, 12, M).astype(np.int64),
             primitive_ids=rng.permutation(M).astype(np.int64), valid_mask=(rng.uniform(0, 1, M) < 0.8).astype(np.uint8),
             cam_mass=rng.uniform(0, 1, M) * (rng.uniform(0, 1, M) > 0.5), lidar_mass=rng.uniform(0, 1, M),
             rgb_cam_accum=rng.uniform(0, 1, (M, 3)), rgb_cam_denom=rng.uniform(0, 1, M))
    return f


def _device_map(ctx, inp, n_tiles, m_tile):
    from gcslam.association import tile_id_from_cell_3d
    from gcslam.primitive_map import DevicePrimitiveMap
    dm = DevicePrimitiveMap(n_tiles, m_tile, ctx=ctx)
    dm.set_tile_keys([tile_id_from_cell_3d(*c) for c in MAP_CELLS[:n_tiles]])
    dm.upload(**{k[4:]: v for k, v in inp.items() if k.startswith("map_")})
    valid = inp["map_valid_mask"].reshape(n_tiles, m_tile)
    dm.tile_count = {d: int(valid[d].sum()) for d in range(n_tiles)}
    dm.total_count = int(valid.sum())
    dm.next_global_id = 1000
    return dm


def _meas(rng, n, x_hi):
    pos = np.column_stack([rng.uniform(0.0, x_hi, n), rng.uniform(0.0, 2.0, n), rng.uniform(0.0, 2.0, n)])
    Lam = _spd(rng, n, 0.2, 4.0)
    return dict(Lambdas=Lam, thetas=np.einsum("nij,nj->ni", Lam, pos), etas=rng.normal(size=(n, L, 3)) * 2.0,
                weights=rng.uniform(0.1, 1.0, n), valid_mask=rng.uniform(0, 1, n) < 0.85,
                colors=rng.uniform(-0.1, 1.1, (n, 3)), sources=(rng.uniform(0, 1, n) < 0.6).astype(np.int32))


# --------------------------------------------------------------------------------------------- OT
OT_H_TILE = 2.5
OT_CFG = dict(k_assoc=6, k_sinkhorn=40, beta=0.6, epsilon=0.12, tau_a=0.45, tau_b=0.55, cost_subtract_row_min=False,
              eps_mass=3e-12, h_tile=OT_H_TILE, r_stencil_tiles_xy=2, r_stencil_tiles_z=1, scan_seq=14,
              recency_decay_lambda=0.03)  # and a_policy WEIGHT_PROPORTIONAL, eps_lift 2e-9
OT_EPS_LIFT = 2e-9


def in_ot():
    rng = np.random.default_rng(101)
    out = {"map_" + k: v for k, v in _map_fields(rng, 2, MAP_M, OT_H_TILE).items()}
    out.update({"meas_" + k: v for k, v in _meas(rng, 32, 4.0 * OT_H_TILE).items()})
    return out


def run_ot(ctx, inp):
    from gcslam.association import (AssociationConfig, MeasurementMassPolicy, associate_primitives_ot,
                                    extract_atlas_map_view)
    dm = _device_map(ctx, inp, 2, MAP_M)
    view = extract_atlas_map_view(dm, dm.tile_keys, 16)
    meas = _Obj(**{k[5:]: v for k, v in inp.items() if k.startswith("meas_")})
    res, cert, eff = associate_primitives_ot(
        meas, view, AssociationConfig(a_policy=MeasurementMassPolicy.WEIGHT_PROPORTIONAL, **OT_CFG), eps_lift=OT_EPS_LIFT)
    out = {k: getattr(res, k) for k in ("responsibilities", "candidate_pool_indices", "candidate_tile_ids",
                                        "candidate_slots", "row_masses", "cost_matrix")}
    ot = cert.ot
    out["cert"] = np.array([ot.marginal_defect_a, ot.marginal_defect_b, ot.transport_mass_total, ot.sum_a, ot.sum_b,
                            ot.sum_m, ot.sum_novel, cert.support.ess_total, ot.nonzero_a, ot.nonzero_b, eff.realized],
                           np.float64)
    return out


# --------------------------------------------------------------------------------------------- map update
MU_H_TILE = 2.5
MU_CFG = dict(k_insert_tile=5, h_tile=MU_H_TILE, block_size=12, eps_lift=2e-9, eps_mass=3e-12, recency_decay_lambda=0.03)
MU_TIMESTAMP, MU_SCAN_SEQ = 12.5, 14


def in_mapupdate():
    from gcslam.association import tile_id_from_cell_3d
    rng = np.random.default_rng(103)
    n, k = 32, 4
    out = {"map_" + k_: v for k_, v in _map_fields(rng, 2, MAP_M, MU_H_TILE).items()}
    out.update({"meas_" + k_: v for k_, v in _meas(rng, n, 4.0 * MU_H_TILE).items()})
    keys = np.array([tile_id_from_cell_3d(*c) for c in MAP_CELLS], np.int64)
    resp = rng.uniform(0.0, 1.0, (n, k))
    out["assoc_responsibilities"] = resp / (4.0 * resp.sum(axis=1, keepdims=True))
    out["assoc_candidate_tile_ids"] = keys[rng.integers(0, 2, (n, k))]
    out["assoc_candidate_slots"] = rng.integers(0, MAP_M, (n, k)).astype(np.int64)
    out["assoc_row_masses"] = rng.uniform(0.0, 0.04, n)
    out["pose"] = np.array([0.05, -0.03, 0.02, 0.01, -0.02, 0.04])
    return out


def run_mapupdate(ctx, inp):
    from gcslam.association import PrimitiveAssociationResult
    from gcslam.primitive_map import MapUpdateConfig, primitive_map_update_from_association
    dm = _device_map(ctx, inp, 2, MAP_M)
    n, k = inp["assoc_responsibilities"].shape
    assoc = PrimitiveAssociationResult(
        responsibilities=inp["assoc_responsibilities"], candidate_pool_indices=np.zeros((n, k), np.int32),
        candidate_tile_ids=inp["assoc_candidate_tile_ids"], candidate_slots=inp["assoc_candidate_slots"],
        row_masses=inp["assoc_row_masses"], cost_matrix=np.zeros((n, k)))
    meas = _Obj(**{k_[5:]: v for k_, v in inp.items() if k_.startswith("meas_")})
    res, _, _ = primitive_map_update_from_association(dm, assoc, meas, dm.tile_keys, inp["pose"], MU_TIMESTAMP,
                                                      MU_SCAN_SEQ, MapUpdateConfig(**MU_CFG), maintenance=False)
    out = {k_: np.asarray(getattr(res, k_)) for k_ in ("insert_indices", "insert_valid", "insert_target_slots", "new_ids")}
    out["counts"] = np.array([res.n_fused, res.n_inserted], np.int64)
    out["masses"] = np.array([res.fused_mass_total, res.insert_mass_total, res.insert_mass_p95], np.float64)
    out.update({"map_" + k_: v for k_, v in dm.download().items()})
    return out


# --------------------------------------------------------------------------------------------- maintenance
MM_CFG = dict(primitive_cull_weight_threshold=0.02, primitive_forgetting_factor=0.98, primitive_merge_threshold=1.5,
              eps_psd=2e-12, eps_lift=3e-9, k_merge_pairs_tile=8, max_tile_size=64)


def in_maintain():
    rng = np.random.default_rng(105)
    return {"map_" + k: v for k, v in _map_fields(rng, 2, MAP_M, 1.0).items()}


def run_maintain(ctx, inp):
    from gcslam.primitive_map import MapUpdateConfig, primitive_map_maintain
    dm = _device_map(ctx, inp, 2, MAP_M)
    res, _, _ = primitive_map_maintain(dm, [1, 0], MapUpdateConfig(**MM_CFG))
    out = dict(n_culled=res.n_culled, mass_dropped=res.mass_dropped, n_merged=res.n_merged)
    out.update({"map_" + k: v for k, v in dm.download().items()})
    return out


# --------------------------------------------------------------------------------------------- surfels
SURFEL_CFG = dict(n_surfel=24, n_feat=7, voxel_size_m=0.3, hex3d_num_cells_1=4, hex3d_num_cells_2=4, hex3d_num_cells_z=2,
                  hex3d_max_occupants=12, min_points_per_voxel=5, sensor_noise_var_per_axis=2e-6, wishart_nu=6.0,
                  wishart_psi_scale=0.15, kappa_main_scale=8.0, kappa_min=0.2, kappa_max=90.0, eig_min=2e-12,
                  eps_lift=3e-9)


def in_surfel():
    rng = np.random.default_rng(107)
    n = 512
    xy = rng.uniform(-0.6, 0.6, (n, 2))
    z = np.where(np.arange(n) % 2 == 0, -0.2, 0.3 * xy[:, 0] + 0.2 * xy[:, 1] + 0.25)
    pts = np.column_stack([xy, z]) + rng.normal(scale=0.003, size=(n, 3))
    pts[::97] = 1e6  # the parser's non-finite sentinel
    return dict(points=pts, timestamps=rng.uniform(0.0, 0.1, n), weights=rng.uniform(0.2, 1.0, n))


def _batch_out(batch):
    from gcslam.measurement_batch import BATCH_ARRAYS
    return {k: np.asarray(getattr(batch, k)) for k in BATCH_ARRAYS}


def run_surfel(ctx, inp):
    from gcslam.ops import SurfelExtractionConfig, extract_lidar_surfels
    batch, _, _ = extract_lidar_surfels(inp["points"], inp["timestamps"], inp["weights"],
                                        SurfelExtractionConfig(**SURFEL_CFG), ctx=ctx)
    out = _batch_out(batch)
    out["lidar_slot_cells"] = np.asarray(batch.lidar_slot_cells)
    out["n_lidar_valid"] = np.asarray(batch.n_lidar_valid)
    return out


# --------------------------------------------------------------------------------------------- camera splats
CAM_K = (25.0, 26.0, 16.0, 12.0)  # a 32 x 24 image
CAM_CFG = dict(depth_fusion_weight_camera=0.9, depth_fusion_weight_lidar=1.1, gamma_lidar=0.8,
               lidar_projection_radius_pix=4.5, lidar_plane_fit_min_points=5, lidar_depth_base_sigma_m=0.03,
               depth_var_min_m2=2e-8, point_support_n0=2.5, point_support_alpha=1.2, spread_mad_beta=9.0, repr_gamma=11.0,
               lidar_ray_plane_fit_max_points=16, plane_intersection_delta=2e-6, plane_angle_sigmoid_alpha=12.0,
               plane_angle_sigmoid_t=0.15, plane_planarity_sigmoid_beta=6.0, plane_planarity_rho0=0.35,
               plane_residual_exp_gamma=90.0, plane_fit_eps=2e-12, depth_min_m=0.06, depth_sigma_max_sq=2e4,
               depth_min_sigmoid_alpha_z=18.0)
CAM_ARGS = dict(pixel_sigma=1.4, n_feat=6, n_surfel=2, eps_lift=2e-9)
CAM_TIMESTAMP = 1712.125
_FEATURE_FIELDS = ("u", "v", "depth_Lambda_c", "depth_theta_c", "weight", "kappa_app", "mu_app", "has_mu_app", "color",
                   "has_color", "xyz", "cov_xyz")


def in_cam():
    rng = np.random.default_rng(109)
    n, m = 256, 8
    fx, fy, cx, cy = CAM_K
    u, v = rng.uniform(0.0, 32.0, n), rng.uniform(0.0, 24.0, n)
    dx, dy = (u - cx) / fx, (v - cy) / fy
    z = np.where(u < 16.0, 4.0, 3.0 / (1.0 - 0.5 * dx)) * (1.0 + 0.0025 * rng.standard_normal(n))
    p_cam = np.column_stack([dx * z, dy * z, z])
    p_cam[:8] *= -1.0  # behind the camera
    c, s = 0.9950041652780258, 0.09983341664682815  # cos, sin of 0.1
    R = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    t = np.array([0.21, -0.04, 0.35])
    i = np.arange(m)
    z_c = rng.uniform(2.0, 6.0, m)
    Lc = np.where(i % 2 == 1, 0.0, 1.0 / (0.05 * z_c) ** 2)
    mu = rng.standard_normal((m, 3))
    mu /= np.sqrt((mu * mu).sum(axis=1))[:, None]
    out = dict(points_base=p_cam @ R.T + t, R=R, t=t, feat_u=rng.uniform(4.0, 28.0, m), feat_v=rng.uniform(4.0, 20.0, m),
               feat_depth_Lambda_c=Lc, feat_depth_theta_c=Lc * z_c, feat_weight=rng.uniform(0.2, 1.0, m),
               feat_kappa_app=rng.uniform(0.5, 20.0, m), feat_mu_app=mu * (i % 3 != 2)[:, None], feat_has_mu_app=i % 3 != 2,
               feat_color=rng.uniform(-0.1, 1.1, (m, 3)), feat_has_color=i % 4 != 3, feat_xyz=rng.uniform(0.5, 5.0, (m, 3)),
               feat_cov_xyz=_spd(rng, m, 0.05, 1e-3))
    return out


def run_cam(ctx, inp):
    from gcslam.ops import CameraFeatures, LidarCameraDepthFusionConfig, PinholeIntrinsics, camera_measurement_batch
    feats = CameraFeatures(**{k: inp["feat_" + k] for k in _FEATURE_FIELDS})
    batch, diag = camera_measurement_batch(inp["points_base"], feats, PinholeIntrinsics(*CAM_K), inp["R"], inp["t"],
                                           CAM_TIMESTAMP, LidarCameraDepthFusionConfig(**CAM_CFG), ctx=ctx,
                                           return_diag=True, **CAM_ARGS)
    out = _batch_out(batch)
    out.update({"diag_" + k: np.asarray(getattr(diag, k)) for k in diag.__dataclass_fields__})
    return out


# --------------------------------------------------------------------------------------------- camera features
CAMFEAT_K = (50.0, 52.0, 32.0, 24.0)
CAMFEAT_CFG = dict(depth_sample_mode="hex", pixel_sigma=1.3, depth_model="quadratic", depth_sigma0=0.012,
                   depth_sigma_slope=0.013, min_depth_m=0.07, max_depth_m=70.0, depth_validity_slope=4.5,
                   response_soft_scale=45.0, depth_scale=1.05, invalid_cov_inflate=2e6, hex_radius=3, quad_fit_radius=1,
                   quad_fit_min_points=5, quad_fit_lstsq_eps=2e-8, student_t_nu=3.5, student_t_w_min=0.15, ma_tau=9.0,
                   ma_delta_inflate=2e-4, kappa0=1.2, kappa_alpha=0.5, kappa_max=90.0, kappa_min=0.2)


def in_camfeat():
    rng = np.random.default_rng(111)
    H, W, m = 48, 64, 16
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    z = np.where(u < 30.0, 4.0 - 0.01 * v, 3.0 / (1.0 - 0.5 * (u - 32.0) / 50.0))
    z[v >= 40.0] = 30.0
    z *= 1.0 + 0.004 * rng.standard_normal((H, W))
    d = z.astype(np.float32)
    bad = rng.uniform(size=(H, W)) < 0.06
    d[bad] = rng.choice(np.array([0.0, np.nan, np.inf, -1.0], np.float32), size=int(bad.sum()))
    d[8:16, 40:48] = 0.0  # a dead block
    uv = np.column_stack([rng.uniform(-1.0, W, m), rng.uniform(-1.0, H, m)])
    uv[0] = [43.6, 12.1]  # in the dead block
    return dict(depth=d, rgb=rng.integers(0, 256, (H, W, 3), dtype=np.uint8), uv=uv, response=rng.uniform(5.0, 150.0, m))


def run_camfeat(ctx, inp):
    from gcslam.ops import VisualFeatureConfig, lift_camera_features
    f = lift_camera_features(inp["depth"], inp["rgb"], inp["uv"], inp["response"], CAMFEAT_K,
                             VisualFeatureConfig(**CAMFEAT_CFG), ctx=ctx)
    return {k: np.asarray(getattr(f, k)) for k in _FEATURE_FIELDS + ("aux",)}


# --------------------------------------------------------------------------------------------- keypoints
KP_CFG = dict(max_features=24, scale_factor=1.3, n_levels=2, edge_threshold=6, fast_threshold=15, harris_k=0.05)


def in_kp():
    return dict(image=np.random.default_rng(113).integers(0, 256, (48, 64, 3), dtype=np.uint8))


def run_kp(ctx, inp):
    from gcslam.ops import OrbDetectorConfig, detect_keypoints
    kp, pyr = detect_keypoints(inp["image"], OrbDetectorConfig(**KP_CFG), ctx=ctx, return_pyramid=True)
    out = {k: np.asarray(getattr(kp, k)) for k in ("uv", "response", "level", "xy_level", "fast_score", "counts")}
    out.update({f"pyramid_{i}": np.asarray(p) for i, p in enumerate(pyr)})
    return out


# --------------------------------------------------------------------------------------------- rendering
RENDER_H = RENDER_W = 32
BEV_CFG = dict(tile_size=16, max_splats_per_tile=4, fbm_octaves=3, fbm_gain=0.6, opacity_gamma=0.8, logdet0=-2.0,
               eps=2e-12, ewa_log_clip=20.0, alpha_min=0.05)
BEV_VIEWPORT = dict(origin_xy=(-1.5, -2.5), px_per_m=7.0, height=RENDER_H, width=RENDER_W)
BEV_ARGS = dict(fbm_seed=11, fbm_modulate_scale=0.3)
BEV_PHI_DEG = 12.0
CAMVIEW_CFG = dict(tile_size=16, max_splats_per_tile=4, near=0.3, far=7.0, lowpass_px2=0.4, radius_sigma=2.5,
                   alpha_floor=0.02, alpha_max=0.9, alpha_skip=1.0 / 128.0, t_stop=1e-3, background=(0.25, 0.5, 0.75),
                   shade=False, eps=2e-12)
CAMVIEW_K = (30.0, 32.0, 16.0, 15.0)


def _in_batch(seed, camera):
    rng = np.random.default_rng(seed)
    n = 32
    if camera:  # in front of an identity camera, a few beyond far
        z = rng.uniform(2.0, 8.0, n)
        mu = np.column_stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.5, 0.5, n) * z, z])
    else:
        mu = np.column_stack([rng.uniform(-1.5, 3.0, n), rng.uniform(-2.5, 2.0, n), rng.uniform(0.0, 1.0, n)])
    return dict(mu_world=mu, Sigma_world=_spd(rng, n, 0.15, 0.01), eta=rng.normal(size=(n, L, 3)) * 2.0,
                mass=rng.uniform(0.05, 1.0, n), color=rng.uniform(0.0, 1.0, (n, 3)))


def in_bev():
    return _in_batch(115, False)


def in_camview():
    out = _in_batch(117, True)
    c, s = 0.9887710779360422, 0.14943813247359922  # cos, sin of 0.15
    T = np.eye(4)
    T[:3, :3] = [[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]
    T[:3, 3] = [0.3, -0.2, 0.5]
    out["T_cw"] = T
    return out


def _render_batch(ctx, inp):
    from gcslam.rendering import DeviceRenderableBatch, RenderablePrimitiveBatch
    n = inp["mu_world"].shape[0]
    return DeviceRenderableBatch.from_host(ctx, RenderablePrimitiveBatch(
        mu_world=inp["mu_world"], Sigma_world=inp["Sigma_world"], Lambda_world=None, eta=inp["eta"], mass=inp["mass"],
        color=inp["color"], primitive_ids=np.arange(n, dtype=np.int64), last_supported_scan_seq=np.zeros(n, np.int64)))


def run_bev(ctx, inp):
    from gcslam import rendering as R
    cfg = R.SplatRenderingConfig(**BEV_CFG)
    P, vd = R.bev_views(R.BEVPushforwardConfig(oblique_phi_deg=BEV_PHI_DEG), "single")
    splats = R.bev_splat_prep(_render_batch(ctx, inp), R.Viewport(**BEV_VIEWPORT), P, vd, cfg, with_sigma_bev=True,
                              **BEV_ARGS)
    dev = R.render_ewa_tiles(splats, RENDER_H, RENDER_W, cfg.tile_size, cfg.max_splats_per_tile, cfg.ewa_log_clip, cfg.eps,
                             ctx=ctx)
    return {k: v.download() for k, v in dict(splats, **dev).items()}


def run_camview(ctx, inp):
    from gcslam import rendering as R
    from gcslam.ops import PinholeIntrinsics
    cfg = R.CameraViewConfig(**CAMVIEW_CFG)
    splats = R.camera_splat_prep(_render_batch(ctx, inp), PinholeIntrinsics(*CAMVIEW_K), inp["T_cw"], RENDER_H, RENDER_W, cfg)
    dev = R.render_depth_tiles(splats, RENDER_H, RENDER_W, cfg, ctx=ctx)
    return {k: v.download() for k, v in dict(splats, **dev).items()}


# name -> (inputs from seeds, the operator on those inputs)
OPS = dict(pipeline=(in_pipeline, run_pipeline), mapupdate=(in_mapupdate, run_mapupdate), maintain=(in_maintain, run_maintain),
           ot=(in_ot, run_ot), surfel=(in_surfel, run_surfel), cam=(in_cam, run_cam), camfeat=(in_camfeat, run_camfeat),
           kp=(in_kp, run_kp), bev=(in_bev, run_bev), camview=(in_camview, run_camview))


def inputs_of(gold, name):
    pre = f"in/{name}/"
    return {k[len(pre):]: gold[k] for k in gold.files if k.startswith(pre)}


def same_bytes(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    from gcslam import _abi
    ctx = _abi.default_context()
    twice = "--twice" in sys.argv[1:]
    out = {}
    for name, (make, run) in OPS.items():
        inp = {k: np.asarray(v) for k, v in make().items()}
        got = {k: np.asarray(v) for k, v in run(ctx, inp).items()}
        assert got, name
        if twice:
            again = run(ctx, inp)
            diff = [k for k in got if not same_bytes(got[k], again[k])]
            print(f"{name}: second run {'identical' if not diff else 'DIFFERS in ' + ', '.join(diff)}")
        out.update({f"in/{name}/{k}": v for k, v in inp.items()})
        out.update({f"out/{name}/{k}": v for k, v in got.items()})
    np.savez_compressed(OUT, **out)
    print(len(out), "arrays,", os.path.getsize(OUT), "bytes")
    for k, v in out.items():
        if k.startswith("out/"):
            f = v.astype(np.float64).reshape(-1)
            fin = f[np.isfinite(f)]
            print(k, v.dtype, v.shape, "nonzero", int(np.count_nonzero(f)), "finite", fin.size,
                  "absmax %.6g" % (float(np.max(np.abs(fin))) if fin.size else 0.0))


if __name__ == "__main__":
    main()
