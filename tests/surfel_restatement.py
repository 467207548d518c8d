"""A NumPy restatement of the reference's LiDAR surfel extraction, in the reference's own form: a
stable argsort for the bucket, gathered (n_cells, max_occupants) point blocks, np.linalg.eigh and
np.linalg.inv. It shares nothing with the device kernels (gc_surfel.hip: a counting sort cut off at
max_occupants, one lane per cell, Jacobi eigh3, LU inv3), so the two are independent routes to the
same numbers.

The reference ships no test vectors for this operator, only the property test
test/test_lidar_surfel_extraction_mahex3d.py: parity is pinned by this restatement ("parity
unpinned" against reference outputs), as VisualPoseEvidence's is by vpe_restatement.py.

    hex_cell_3d_batch, bin_points_3d          common/ma_hex_web.py:221-303
    _normalize, basis, _fit_one_cell          backend/operators/lidar_surfel_extraction.py:69-163
    mask, centre, select, zeroed tail         lidar_surfel_extraction.py:255-331
    create_empty_measurement_batch            backend/structures/measurement_batch.py:137-157
    grey from n_z, add_lidar_surfels          measurement_batch.py:262-347

Besides the batch, `extract` returns what the tests' preconditions need: per cell the eigenvalues and
the occupancy before and after clipping, per point the distance of s/h from the nearest integer."""

import numpy as np

SENTINEL = 1e6   # GC_NONFINITE_SENTINEL, common/constants.py:257
N_LOBES = 3      # GC_VMF_N_LOBES, common/constants.py:463
EPS = 1e-12      # _fit_one_cell's and _normalize's eps default (:69, :99)

DEFAULTS = dict(n_surfel=1024, n_feat=512, voxel_size_m=0.1, hex3d_num_cells_1=32, hex3d_num_cells_2=32,
                hex3d_num_cells_z=8, hex3d_max_occupants=32, min_points_per_voxel=3, sensor_noise_var_per_axis=1e-6,
                wishart_nu=5.0, wishart_psi_scale=0.1, kappa_main_scale=10.0, kappa_min=0.1, kappa_max=100.0,
                eig_min=1e-12, eps_lift=1e-9)  # SurfelExtractionConfig, :43-62


def hex_coords(points_c, h):
    """ma_hex_web.py:233-239 before the floor: s / h on the three axes, (N, 3)."""
    h = max(float(h), 1e-12)
    s1 = points_c[:, 0]
    s2 = points_c[:, 0] * 0.5 + points_c[:, 1] * (np.sqrt(3.0) * 0.5)
    return np.stack([s1 / h, s2 / h, points_c[:, 2] / h], axis=1)


def bin_points_3d(points_c, mask, cfg):
    """ma_hex_web.py:243-303: (bucket (n_cells, max_occ) of point indices, -1 = empty; count; clipped count)."""
    n1, n2, nz = cfg["hex3d_num_cells_1"], cfg["hex3d_num_cells_2"], cfg["hex3d_num_cells_z"]
    n_cells, max_occ, N = n1 * n2 * nz, cfg["hex3d_max_occupants"], points_c.shape[0]
    with np.errstate(invalid="ignore"):
        cells = np.floor(hex_coords(points_c, cfg["voxel_size_m"])).astype(np.int64).astype(np.int32)
    cells = np.mod(cells, np.array([n1, n2, nz], np.int32)[None, :])  # floor-mod: non-negative
    linear = (cells[:, 0] * (n2 * nz) + cells[:, 1] * nz + cells[:, 2]).astype(np.int32)
    m = mask.astype(np.int32)
    linear = np.where(m > 0, linear, 0)
    order = np.argsort(linear + (1 - m) * n_cells, kind="stable")  # masked points last (:275-277)
    linear_s, mask_s, idx_s = linear[order], m[order], np.arange(N, dtype=np.int32)[order]
    pos = np.arange(N, dtype=np.int32)
    count = np.zeros(n_cells, np.int32)
    np.add.at(count, linear_s, mask_s)
    start = np.full(n_cells, N, np.int32)
    np.minimum.at(start, linear_s, pos)
    start = np.where(count > 0, start, 0)
    rank = pos - start[linear_s]
    keep = (mask_s == 1) & (rank < max_occ)
    bucket_ext = np.full((n_cells + 1, max_occ + 1), -1, np.int32)
    bucket_ext[np.where(keep, linear_s, n_cells), np.where(keep, rank, max_occ)] = np.where(keep, idx_s, -1)
    return bucket_ext[:n_cells, :max_occ], count, np.minimum(count, max_occ)


def _normalize(v):
    return v / (np.linalg.norm(v, axis=-1, keepdims=True) + EPS)


def fit_cells(points_c, timestamps, weights_eff, bucket, count_used, cfg):
    """_fit_one_cell (:84-163) over every cell at once (the reference vmaps it, :294)."""
    eig_min, I = cfg["eig_min"], np.eye(3)
    present = (bucket >= 0).astype(np.float64)
    safe = np.maximum(bucket, 0)
    pts = points_c[safe]                                  # (C, M, 3)
    w = weights_eff[safe] * present
    t = timestamps[safe] * present                        # not weighted (:119)
    w_sum = w.sum(axis=1) + EPS
    centroid = (pts * w[..., None]).sum(axis=1) / w_sum[:, None]
    centered = pts - centroid[:, None, :]
    cov = np.einsum("cmi,cmj->cij", centered * w[..., None], centered) / w_sum[:, None, None]
    cov = 0.5 * (cov + np.swapaxes(cov, 1, 2)) + eig_min * I
    eigvals, eigvecs = np.linalg.eigh(cov)
    normal = eigvecs[:, :, 0]
    normal = normal * np.where(normal[:, 2:3] < 0.0, -1.0, 1.0)
    normal = _normalize(normal)
    n2 = _normalize(normal)                               # the basis normalises once more (:74)
    e1 = np.where((np.abs(n2[:, 2]) < 0.9)[:, None],
                  np.stack([-n2[:, 1], n2[:, 0], np.zeros(len(n2))], axis=1),
                  np.stack([-n2[:, 2], np.zeros(len(n2)), n2[:, 0]], axis=1))
    e1 = _normalize(e1)
    e2 = _normalize(np.cross(n2, e1))
    proj1 = np.einsum("cmi,ci->cm", centered, e1)
    proj2 = np.einsum("cmi,ci->cm", centered, e2)
    sensor = cfg["sensor_noise_var_per_axis"]
    var_e1 = (w * proj1 * proj1).sum(axis=1) / w_sum + sensor
    var_e2 = (w * proj2 * proj2).sum(axis=1) / w_sum + sensor
    sigma_perp_sq = np.maximum(eigvals[:, 0], eig_min)
    var_perp = sigma_perp_sq + sensor
    V = np.stack([e1, e2, normal], axis=2)
    D = np.maximum(np.stack([var_e1, var_e2, var_perp], axis=1), eig_min)
    Sigma = np.einsum("cik,ck,cjk->cij", V, D, V)
    Sigma = 0.5 * (Sigma + np.swapaxes(Sigma, 1, 2)) + eig_min * I
    Lam = np.linalg.inv(Sigma + eig_min * I)
    Lam = 0.5 * (Lam + np.swapaxes(Lam, 1, 2))
    Lam_reg = Lam + (cfg["wishart_nu"] / max(cfg["wishart_psi_scale"], EPS)) * I
    Lam_reg = 0.5 * (Lam_reg + np.swapaxes(Lam_reg, 1, 2)) + eig_min * I
    Sigma_reg = np.linalg.inv(Lam_reg)
    Sigma_reg = 0.5 * (Sigma_reg + np.swapaxes(Sigma_reg, 1, 2)) + eig_min * I
    kappa = np.clip(cfg["kappa_main_scale"] / np.sqrt(np.maximum(sigma_perp_sq, eig_min)),
                    cfg["kappa_min"], cfg["kappa_max"])
    w_surfel = w.sum(axis=1)
    t_surfel = t.sum(axis=1) / w_sum
    valid = (count_used >= cfg["min_points_per_voxel"]) & (w_surfel > 0.0)
    return dict(centroid=centroid, Sigma_reg=Sigma_reg, normal=normal, kappa=kappa, w=w_surfel, t=t_surfel,
                valid=valid, eigvals=eigvals)


def extract(points, timestamps, weights, config=None, base=None):
    """extract_lidar_surfels (:339-431) -> a dict of the nine batch arrays, the counts and diagnostics.
    base: a dict of the nine arrays plus n_camera_valid to add the LiDAR slice to (:383-395)."""
    cfg = dict(DEFAULTS, **(config or {}))
    points = np.asarray(points, np.float64).reshape(-1, 3)
    timestamps = np.asarray(timestamps, np.float64).reshape(-1)
    weights = np.asarray(weights, np.float64).reshape(-1)
    mask = np.all(np.abs(points) < 0.1 * SENTINEL, axis=1)               # :261
    weights_eff = weights * mask
    w_sum = weights_eff.sum() + cfg["eig_min"]                           # :265 (eig_min, not eps)
    center = (points * weights_eff[:, None]).sum(axis=0) / w_sum
    points_c = points - center[None, :]
    bucket, count, count_used = bin_points_3d(points_c, mask, cfg)
    fit = fit_cells(points_c, timestamps, weights_eff, bucket, count_used, cfg)
    n_cells, n_surfel, n_feat = bucket.shape[0], cfg["n_surfel"], cfg["n_feat"]
    key = np.arange(n_cells) + (1 - fit["valid"].astype(np.int64)) * n_cells   # :299-302
    take = np.argsort(key, kind="stable")[:n_surfel]
    n_valid = int(fit["valid"][take].sum())
    take = take[:n_valid]
    positions = fit["centroid"][take] + center[None, :]
    # measurement_batch.py:299-312
    Lam_row = np.linalg.inv(fit["Sigma_reg"][take] + cfg["eps_lift"] * np.eye(3)[None])
    thetas = np.einsum("nij,nj->ni", Lam_row, positions)
    normals = fit["normal"][take]
    grey = 0.25 + 0.5 * (np.clip(normals[:, 2:3], -1.0, 1.0) + 1.0) / 2.0
    n_total = n_feat + n_surfel
    if base is None:                                                      # measurement_batch.py:137-157
        out = dict(Lambdas=np.zeros((n_total, 3, 3)), thetas=np.zeros((n_total, 3)),
                   etas=np.zeros((n_total, N_LOBES, 3)), weights=np.zeros(n_total),
                   sources=np.zeros(n_total, np.int32), source_indices=np.zeros(n_total, np.int32),
                   valid_mask=np.zeros(n_total, bool), timestamps=np.zeros(n_total), colors=np.zeros((n_total, 3)))
        n_cam = 0
    else:
        out = {k: np.array(base[k]) for k in ("Lambdas", "thetas", "etas", "weights", "sources", "source_indices",
                                               "valid_mask", "timestamps", "colors")}
        n_cam = int(base["n_camera_valid"])
    rows = slice(n_feat, n_feat + n_valid)                                # :314-331
    out["Lambdas"][rows] = Lam_row
    out["thetas"][rows] = thetas
    out["etas"][rows] = 0.0
    out["etas"][rows, 0, :] = fit["kappa"][take, None] * normals
    out["weights"][rows] = fit["w"][take]
    out["sources"][rows] = 1
    out["source_indices"][rows] = np.arange(n_valid, dtype=np.int32)
    out["valid_mask"][rows] = True
    out["timestamps"][rows] = fit["t"][take]
    out["colors"][rows] = np.broadcast_to(grey, (n_valid, 3))
    # diagnostics
    lam = fit["eigvals"]
    nz = np.abs(fit["normal"][:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        determined = ((lam[:, 1] - lam[:, 0]) / lam[:, 2] >= 1e-4) & (nz >= 1e-6) & (np.abs(nz - 0.9) >= 1e-6)
        sc = hex_coords(points_c, cfg["voxel_size_m"])
        margin = np.abs(sc - np.round(sc)).min(axis=1)
    out.update(n_feat=n_feat, n_surfel=n_surfel, n_camera_valid=n_cam, n_lidar_valid=n_valid, slot_cells=take,
               positions=positions, kappas=fit["kappa"][take], center=center, mask=mask, bucket=bucket,
               count=count, count_used=count_used, cell_valid=fit["valid"], eigvals=lam,
               cell_determined=determined, slot_determined=determined[take], point_margin=margin)
    return out
