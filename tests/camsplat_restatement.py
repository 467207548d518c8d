"""TEST INFRASTRUCTURE — NumPy restatement of the camera-splat path, in its own vectorised form.

  evidence()        lidar_depth_evidence with Route A and Route B
                    (frontend/sensors/lidar_camera_depth_fusion.py:80-442). Pinned: the recorded outputs
                    of the reference's own NumPy code are in tests/golden/camera_splats.npz
                    (tests/golden/make_camera_splats.py) and test_camera_splats.py holds this file to them.
  fuse()            splat_prep_fused's PoE fusion, fall-backs, backprojection and closed-form covariance
                    (frontend/sensors/splat_prep.py:37-134). Pinned the same way.
  to_camera_frame() / to_base_frame()   the node's two frame changes (backend/backend_node.py:1876,
                    :1888-1899). Node code: parity unpinned.
  batch_rows()      feature_list_to_camera_batch + measurement_batch_from_camera_splats
                    (backend/camera_batch_utils.py:23-86, backend/structures/measurement_batch.py:165-259).
                    JAX code in the reference: parity unpinned.

evidence() also returns what the test conditions are stated on: the margin of every (query, point)
pair to the radius, the gap between the k-th and (k+1)-th ray distances, n_z, z_raw and the
eigenvalues of every fitted plane. cfg is any object with the LidarCameraDepthFusionConfig fields."""

from __future__ import annotations

import numpy as np

MAD_NORMAL_SCALE = 1.4826
EV_KEYS = ("Lambda_A", "theta_A", "Lambda_B", "theta_B", "Lambda_ell", "theta_ell", "z_B", "sigma_sq_B", "w_B")


def _sigmoid(x):
    x = float(x)
    if x >= 0:
        return 1.0 / (1.0 + np.exp(-x))
    t = np.exp(x)
    return t / (1.0 + t)


def _softplus(x):
    x = float(x)
    if x > 20.0:
        return x
    if x < -20.0:
        return 0.0
    return float(np.log(1.0 + np.exp(x)))


def to_camera_frame(points_base, R, t):
    p = np.asarray(points_base, np.float64).reshape(-1, 3)
    return (np.asarray(R, np.float64).T @ (p.T - np.asarray(t, np.float64)[:, None])).T if p.shape[0] else p


def project(points_cam, fx, fy, cx, cy):
    p = np.asarray(points_cam, np.float64).reshape(-1, 3)
    z = p[:, 2]
    return fx * (p[:, 0] / (z + 1e-12)) + cx, fy * (p[:, 1] / (z + 1e-12)) + cy, z


def evidence(points_cam, uv_query, fx, fy, cx, cy, cfg, point_weights=None):
    p_all = np.asarray(points_cam, np.float64).reshape(-1, 3)
    q = np.asarray(uv_query, np.float64).reshape(-1, 2)
    M = q.shape[0]
    out = {k: np.zeros(M) for k in EV_KEYS}
    out["z_B"][:] = np.nan
    out["sigma_sq_B"][:] = np.nan
    cond = dict(counts=np.zeros(M, np.int64), radius_margin=np.inf, kth_gap=np.full(M, np.inf),
                n_z=np.full(M, np.nan), z_raw=np.full(M, np.nan), eig=np.full((M, 3), np.nan),
                k_use=np.zeros(M, np.int64), supported=np.zeros(M, bool))
    out["cond"] = cond
    u, v, z = project(p_all, fx, fy, cx, cy)
    front = z > 0.0
    p, u, v, z = p_all[front], u[front], v[front], z[front]
    pw = None if point_weights is None else np.asarray(point_weights, np.float64).ravel()[front]
    n_front = p.shape[0]
    if n_front == 0 or M == 0:
        return out
    r2 = cfg.lidar_projection_radius_pix * cfg.lidar_projection_radius_pix
    d2 = (u[None, :] - q[:, :1]) ** 2 + (v[None, :] - q[:, 1:]) ** 2  # (M, n_front)
    near = d2 <= r2
    cond["counts"][:] = near.sum(axis=1)
    cond["radius_margin"] = float(np.min(np.abs(d2 - r2)) / r2)
    K = min(int(cfg.lidar_ray_plane_fit_max_points), n_front)
    base2 = cfg.lidar_depth_base_sigma_m * cfg.lidar_depth_base_sigma_m
    z_min = cfg.depth_min_m
    for i in range(M):
        idx = np.flatnonzero(near[i])
        n = idx.size
        if n == 0 or n < cfg.lidar_plane_fit_min_points:
            continue
        cond["supported"][i] = True
        # Route A
        zn = z[idx]
        med = float(np.median(zn))
        sA = MAD_NORMAL_SCALE * float(np.median(np.abs(zn - med)))
        var = float(np.var(zn)) if n >= 2 else 0.0
        sig = max(base2 + max(sA * sA, var), cfg.depth_var_min_m2)
        wA = (_sigmoid(cfg.point_support_alpha * (float(n) - cfg.point_support_n0)) * np.exp(-cfg.spread_mad_beta * sA * sA)
              * np.exp(-cfg.repr_gamma * var))
        if not (wA <= 0.0 or not np.isfinite(med) or med <= 0.0):
            out["Lambda_A"][i] = wA / sig
            out["theta_A"][i] = out["Lambda_A"][i] * med
        # Route B (it needs min_points z > 0 points in all, which n >= min_points implies)
        ray = np.array([(q[i, 0] - cx) / fx, (q[i, 1] - cy) / fy, 1.0])
        nr = np.linalg.norm(ray)
        ray = np.array([0.0, 0.0, 1.0]) if nr < 1e-12 else ray / nr
        rd = ray / (np.linalg.norm(ray) + 1e-12)
        pn = p[idx]
        diff = pn - (pn @ rd)[:, None] * rd
        dist = np.sum(diff * diff, axis=1)
        k_use = min(K, n)
        order = np.lexsort((np.arange(n), dist))  # by (distance, point index)
        if n > k_use:
            a, b = dist[order[k_use - 1]], dist[order[k_use]]
            cond["kth_gap"][i] = (b - a) / max(b, 1e-300)
        cond["k_use"][i] = k_use
        sel = order[:k_use]
        pts = pn[sel]
        w = np.ones(k_use) if pw is None else pw[idx][sel]
        sw = float(np.sum(w))
        cen = (pts * w[:, None]).sum(axis=0) / sw
        c = pts - cen
        S = (c.T * w) @ c / (sw + 1e-300)
        S = 0.5 * (S + S.T) + 1e-12 * np.eye(3)
        lam, vec = np.linalg.eigh(S)
        nrm = vec[:, 0]
        if nrm[2] < 0:
            nrm = -nrm
        sp = max(float(np.sum(w * (c @ nrm) ** 2) / sw), 0.0)
        ndr = float(nrm @ ray)
        z_raw = float(nrm @ cen) / (ndr + cfg.plane_intersection_delta)
        cond["n_z"][i], cond["z_raw"][i], cond["eig"][i] = nrm[2], z_raw, lam
        zb = _softplus(z_raw - z_min) + z_min
        w_behind = _sigmoid(z_raw - z_min) if z_raw < z_min else 1.0
        sb = base2 + sp / max(ndr * ndr + cfg.plane_intersection_delta, cfg.plane_intersection_delta)
        sb = min(max(sb, cfg.depth_var_min_m2), cfg.depth_sigma_max_sq)
        l2, l3 = max(lam[1], cfg.plane_fit_eps), max(lam[2], cfg.plane_fit_eps)
        wB = (_sigmoid(cfg.plane_angle_sigmoid_alpha * (abs(ndr) - cfg.plane_angle_sigmoid_t))
              * _sigmoid(cfg.plane_planarity_sigmoid_beta * (float(l2 / (l3 + cfg.plane_fit_eps)) - cfg.plane_planarity_rho0))
              * np.exp(-cfg.plane_residual_exp_gamma * sp) * w_behind)
        wB = max(wB * _sigmoid(cfg.depth_min_sigmoid_alpha_z * (zb - z_min)), 0.0)
        out["z_B"][i], out["sigma_sq_B"][i], out["w_B"][i] = zb, sb, wB
        if np.isfinite(zb) and zb > 0.0 and np.isfinite(sb) and sb > 0.0 and wB > 0.0:
            out["Lambda_B"][i] = wB / max(sb, cfg.depth_var_min_m2)
            out["theta_B"][i] = out["Lambda_B"][i] * zb
    out["Lambda_ell"] = (out["Lambda_A"] + out["Lambda_B"]) * cfg.gamma_lidar
    out["theta_ell"] = (out["theta_A"] + out["theta_B"]) * cfg.gamma_lidar
    return out


def determined(cond, tol=1e-4):
    """Queries whose plane normal is determined: (λ1 − λ0) / λ2 >= tol. Unsupported queries count as
    determined (Route B writes its defaults there)."""
    lam = cond["eig"]
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (lam[:, 1] - lam[:, 0]) / lam[:, 2] >= tol
    return np.where(cond["supported"], ok, True)


def fuse(feat, Lambda_ell, theta_ell, fx, fy, cx, cy, cfg, pixel_sigma=1.0):
    """feat: dict of the CameraFeatures arrays. Returns xyz (M, 3), cov (M, 3, 3), fused (M,) bool."""
    u, v = np.asarray(feat["u"], np.float64), np.asarray(feat["v"], np.float64)
    Lf = cfg.depth_fusion_weight_camera * feat["depth_Lambda_c"] + cfg.depth_fusion_weight_lidar * Lambda_ell
    tf = cfg.depth_fusion_weight_camera * feat["depth_theta_c"] + cfg.depth_fusion_weight_lidar * theta_ell
    ok = ~(Lf <= 0.0) & np.isfinite(Lf) & np.isfinite(tf)
    with np.errstate(all="ignore"):
        zf, sf = tf / Lf, 1.0 / Lf
    ok &= np.isfinite(zf) & ~(zf <= 0.0) & np.isfinite(sf) & ~(sf <= 0.0)
    zf, sf = np.where(ok, zf, 1.0), np.where(ok, sf, 1.0)
    vz = np.maximum(np.maximum(sf, cfg.depth_var_min_m2), 0.0)
    vu = vv = max(pixel_sigma ** 2, 0.0)
    du, dv = u - cx, v - cy
    xyz = np.stack([du * zf / fx, dv * zf / fy, zf], axis=1)
    cov = np.zeros((u.shape[0], 3, 3))
    cov[:, 0, 0] = (zf * zf * vu + du * du * vz + vu * vz) / (fx * fx)
    cov[:, 1, 1] = (zf * zf * vv + dv * dv * vz + vv * vz) / (fy * fy)
    cov[:, 0, 1] = cov[:, 1, 0] = (du * dv * vz) / (fx * fy)
    cov[:, 0, 2] = cov[:, 2, 0] = (du * vz) / fx
    cov[:, 1, 2] = cov[:, 2, 1] = (dv * vz) / fy
    cov[:, 2, 2] = vz
    xyz = np.where(ok[:, None], xyz, feat["xyz"])
    cov = np.where(ok[:, None, None], cov, feat["cov_xyz"])
    return xyz, cov, ok


def to_base_frame(xyz, cov, mu_app, R, t):
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    return xyz @ R.T + t, R @ cov @ R.T, mu_app @ R.T


def batch_rows(positions, covariances, directions, kappas, weights, timestamps, colors, n_feat, n_surfel, eps_lift,
               n_lobes=3):
    """measurement_batch_from_camera_splats: the nine arrays and n_camera_valid."""
    N = positions.shape[0]
    nv, nt = min(N, n_feat), n_feat + n_surfel
    out = dict(Lambdas=np.zeros((nt, 3, 3)), thetas=np.zeros((nt, 3)), etas=np.zeros((nt, n_lobes, 3)),
               weights=np.zeros(nt), sources=np.zeros(nt, np.int32), source_indices=np.zeros(nt, np.int32),
               valid_mask=np.zeros(nt, bool), timestamps=np.zeros(nt), colors=np.zeros((nt, 3)), n_camera_valid=nv)
    if nv:
        L = np.linalg.inv(covariances[:nv] + eps_lift * np.eye(3)[None])
        out["Lambdas"][:nv] = L
        out["thetas"][:nv] = np.einsum("nij,nj->ni", L, positions[:nv])
        out["etas"][:nv, 0] = kappas[:nv, None] * directions[:nv]
        out["weights"][:nv] = weights[:nv]
        out["source_indices"][:nv] = np.arange(nv, dtype=np.int32)
        out["valid_mask"][:nv] = True
        out["timestamps"][:nv] = timestamps[:nv]
        out["colors"][:nv] = np.clip(colors[:nv], 0.0, 1.0) if colors is not None else 0.5
    return out


def camera_batch(feat, xyz_cam, cov_cam, R, t, timestamp_sec, n_feat, n_surfel, eps_lift, n_lobes=3):
    """The node's base-frame loop, then feature_list_to_camera_batch's packing, then batch_rows."""
    M = xyz_cam.shape[0]
    xyz_b, cov_b, mu_b = to_base_frame(xyz_cam, cov_cam, np.asarray(feat["mu_app"], np.float64), R, t)
    d = np.where(np.asarray(feat["has_mu_app"], bool)[:, None], mu_b, xyz_b)
    dirs = d / (np.linalg.norm(d, axis=1) + 1e-12)[:, None]
    colors = np.where(np.asarray(feat["has_color"], bool)[:, None], feat["color"], 0.5)
    return batch_rows(xyz_b, cov_b, dirs, np.asarray(feat["kappa_app"], np.float64),
                      np.asarray(feat["weight"], np.float64), np.full(M, timestamp_sec), colors, n_feat, n_surfel,
                      eps_lift, n_lobes)
