"""A NumPy restatement (f64) of the RGB-D surfel extraction (gc_extract_depth_surfels, include/gcslam.h;
DESIGN.md §4, "Depth surfels"). The operator is this build's, so this file is the statement its device
kernels (gc_depthsurfel.hip: one wave per cell, lane-strided sums and a butterfly, Jacobi eigh3, LU inv3) are
held to: cells, pixel validity, pixel-centre backprojection, the base frame, two-pass moments with unit
weights, the three gates, the even selection and the rows, in whole-image array form.

The plane fit is not rewritten: it is surfel_restatement.fit_cells, the restated _fit_one_cell the LiDAR
extractor is held to, fed the used pixels of every cell as its bucket, unit weights and the per-cell
sigma_z(zbar)^2 as the sensor's variance. fit_cells divides by n + 1e-12 where the operator divides by n: a
relative 1e-14 at n >= 3, four orders under the comparison bar; the row's position, weight and timestamp are
taken from the moments computed here, as specified. The row is the few lines of
measurement_batch_add_lidar_surfels that surfel_restatement.extract holds inline (:138-142), restated."""

import math

import numpy as np

import surfel_restatement as SR

N_LOBES = SR.N_LOBES
DEFAULTS = dict(cell_px=16, min_fill=0.5, min_depth_m=0.05, max_depth_m=80.0, depth_model="linear", depth_sigma0=0.01,
                depth_sigma_slope=0.01, plane_gate=2.0, min_cos_incidence=0.1, weight_scale=1.0,
                **{k: SR.DEFAULTS[k] for k in ("n_surfel", "n_feat", "wishart_nu", "wishart_psi_scale", "kappa_main_scale",
                                               "kappa_min", "kappa_max", "eig_min", "eps_lift")})
ARRAYS = ("Lambdas", "thetas", "etas", "weights", "sources", "source_indices", "valid_mask", "timestamps", "colors")


def select(V: int, free: int) -> np.ndarray:
    """The ranks (among the V valid cells in ascending cell id) that are kept, ascending: all when V <= free,
    otherwise rank r iff floor((r + 1) free / V) > floor(r free / V)."""
    r = np.arange(V, dtype=np.int64)
    if V <= free:
        return r
    return r[((r + 1) * free) // V > (r * free) // V]


def sigma_z(zbar, cfg):
    return cfg["depth_sigma0"] + cfg["depth_sigma_slope"] * (zbar * zbar if cfg["depth_model"] == "quadratic" else zbar)


def min_count(cfg) -> int:
    return max(3, math.ceil(cfg["min_fill"] * float(cfg["cell_px"] ** 2)))


def extract(depth, rgb, intrinsics, R_base_camera=None, t_base_camera=None, timestamp_sec=0.0, config=None, base=None):
    """-> a dict of the nine batch arrays, the counts, slot_cells (n_feat; -1 = not written) and diagnostics.
    intrinsics = (fx, fy, cx, cy); base: a dict of the nine arrays plus n_camera_valid and n_lidar_valid."""
    cfg = dict(DEFAULTS, **(config or {}))
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    R = np.eye(3) if R_base_camera is None else np.asarray(R_base_camera, np.float64)
    t = np.zeros(3) if t_base_camera is None else np.asarray(t_base_camera, np.float64).reshape(3)
    z = np.asarray(depth).astype(np.float64)  # the cases hold float32 depths, what the device reads
    H, W = z.shape
    cell = int(cfg["cell_px"])
    n_cx, n_cy = -(-W // cell), -(-H // cell)
    n_cells, area = n_cx * n_cy, cell * cell
    # pixel validity, backprojection through the pixel centre, the base frame
    with np.errstate(invalid="ignore"):
        used = np.isfinite(z) & (z > cfg["min_depth_m"]) & (z < cfg["max_depth_m"])
    z = np.where(used, z, 0.0)
    i, j = np.mgrid[0:H, 0:W]
    pc = np.stack([z * ((j + 0.5 - cx) / fx), z * ((i + 0.5 - cy) / fy), z], axis=-1)
    pb = (pc @ R.T + t[None, None, :]).reshape(-1, 3)
    cell_id = ((i // cell) * n_cx + (j // cell)).reshape(-1)
    used_f, z_f = used.reshape(-1), z.reshape(-1)
    col = None if rgb is None else np.asarray(rgb, np.uint8).reshape(-1, 3).astype(np.int64)
    # per-cell moments over the used pixels (row-major within the cell), unit weights, two passes
    bucket = np.full((n_cells, area), -1, np.int32)
    n = np.zeros(n_cells, np.int64)
    mean, C, zbar = np.zeros((n_cells, 3)), np.zeros((n_cells, 3, 3)), np.zeros(n_cells)
    col_sum = np.zeros((n_cells, 3), np.int64)
    for c in range(n_cells):
        idx = np.flatnonzero(used_f & (cell_id == c))
        n[c] = idx.size
        bucket[c, :idx.size] = idx
        if idx.size:
            mean[c] = pb[idx].sum(axis=0) / idx.size
            d = pb[idx] - mean[c][None, :]
            C[c] = (d.T @ d) / idx.size
            zbar[c] = z_f[idx].sum() / idx.size
            if col is not None:
                col_sum[c] = col[idx].sum(axis=0)
    sig = sigma_z(zbar, cfg)
    # the plane fit: the LiDAR extractor's restated _fit_one_cell
    fit_cfg = dict(eig_min=cfg["eig_min"], sensor_noise_var_per_axis=sig * sig, wishart_nu=cfg["wishart_nu"],
                   wishart_psi_scale=cfg["wishart_psi_scale"], kappa_main_scale=cfg["kappa_main_scale"],
                   kappa_min=cfg["kappa_min"], kappa_max=cfg["kappa_max"], min_points_per_voxel=min_count(cfg))
    N = pb.shape[0]
    fit = SR.fit_cells(pb, np.full(N, float(timestamp_sec)), np.ones(N), bucket, n, fit_cfg)
    normal = fit["normal"]
    # the gates
    fill_ok = n >= min_count(cfg)
    lam_min = np.linalg.eigvalsh(C)[:, 0]
    plane_thr = (cfg["plane_gate"] * sig) ** 2
    plane_ok = lam_min <= plane_thr
    ray = mean - t[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        cos_inc = np.abs(np.einsum("ci,ci->c", normal, ray)) / np.linalg.norm(ray, axis=1)
    inc_ok = cos_inc >= cfg["min_cos_incidence"]
    valid = fill_ok & plane_ok & inc_ok
    # the selection and the rows
    n_feat, n_surfel = int(cfg["n_feat"]), int(cfg["n_surfel"])
    n_total = n_feat + n_surfel
    if base is None:
        out = dict(Lambdas=np.zeros((n_total, 3, 3)), thetas=np.zeros((n_total, 3)), etas=np.zeros((n_total, N_LOBES, 3)),
                   weights=np.zeros(n_total), sources=np.zeros(n_total, np.int32),
                   source_indices=np.zeros(n_total, np.int32), valid_mask=np.zeros(n_total, bool),
                   timestamps=np.zeros(n_total), colors=np.zeros((n_total, 3)))
        n_in, n_lidar = 0, 0
    else:
        out = {k: np.array(base[k]) for k in ARRAYS}
        n_in, n_lidar = int(base["n_camera_valid"]), int(base.get("n_lidar_valid", 0))
    free = n_feat - n_in
    valid_cells = np.flatnonzero(valid)
    take = valid_cells[select(valid_cells.size, free)]
    n_new = take.size
    rows = np.arange(n_in, n_in + n_new)
    # measurement_batch.py:299-312, as surfel_restatement.extract restates it
    Lam_row = np.linalg.inv(fit["Sigma_reg"][take] + cfg["eps_lift"] * np.eye(3)[None])
    positions = mean[take]
    grey = 0.25 + 0.5 * (np.clip(normal[take, 2:3], -1.0, 1.0) + 1.0) / 2.0
    out["Lambdas"][rows] = Lam_row
    out["thetas"][rows] = np.einsum("nij,nj->ni", Lam_row, positions)
    out["etas"][rows] = 0.0
    out["etas"][rows, 0, :] = fit["kappa"][take, None] * normal[take]
    out["weights"][rows] = cfg["weight_scale"] * n[take].astype(np.float64) / float(area)
    out["sources"][rows] = 0
    out["source_indices"][rows] = rows.astype(np.int32)
    out["valid_mask"][rows] = True
    out["timestamps"][rows] = float(timestamp_sec)
    if col is None:
        out["colors"][rows] = np.broadcast_to(grey, (n_new, 3))
    else:
        out["colors"][rows] = col_sum[take].astype(np.float64) / (255.0 * n[take].astype(np.float64))[:, None]
    slot_cells = np.full(n_feat, -1, np.int32)
    slot_cells[rows] = take
    # diagnostics: the orientation criteria of surfel_restatement.extract, the gates' distances from their thresholds
    lam = fit["eigvals"]
    nz = np.abs(normal[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        determined = ((lam[:, 1] - lam[:, 0]) / lam[:, 2] >= 1e-4) & (nz >= 1e-6) & (np.abs(nz - 0.9) >= 1e-6)
        plane_margin = np.abs(lam_min - plane_thr) / plane_thr
        inc_margin = np.abs(cos_inc - cfg["min_cos_incidence"])
    out.update(n_feat=n_feat, n_surfel=n_surfel, n_camera_valid=n_in + n_new, n_lidar_valid=n_lidar, n_new=n_new,
               n_in=n_in, free=free, slot_cells=slot_cells, kept_cells=take, rows=rows, positions=positions,
               kappas=fit["kappa"][take], n_cells=n_cells, n_cx=n_cx, cell_n=n, cell_mean=mean, cell_cov=C,
               cell_zbar=zbar, cell_normal=normal, cell_fill_ok=fill_ok, cell_plane_ok=plane_ok, cell_inc_ok=inc_ok,
               cell_valid=valid, cell_determined=determined, slot_determined=determined[take],
               plane_margin=plane_margin, inc_margin=inc_margin, eigvals=lam)
    return out
