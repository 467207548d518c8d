"""TEST INFRASTRUCTURE — NumPy restatement of the visual feature node's per-keypoint arithmetic, in its
own vectorised form (all keypoints at once, windows as masked (M, P) arrays, medians by a masked
sort, the fits by one batched np.linalg.solve).

  lift()   depth_sample / depth_sample_hex (src/visual_feature_node.cpp:228-348), validate_depth,
           depth_weight, response_weight, depth_sigma (:184-226), student_t_effective_var (:350-369),
           backproject, backprojection_cov (:371-399), quadratic_fit (:401-491), the per-feature
           assembly (:547-634), and what _feature_batch_to_list makes of the message
           (backend/backend_node.py:1600-1601, :1616-1620).

Parity unpinned: the reference ships no recorded vectors for this node, and the node cannot be built
without ROS 2 and OpenCV, so nothing holds this file to the C++ but the reading of it cited line by
line below; test_camera_features.py checks it against analytic answers.

Where the C++ leaves an order open (the sums over zs run after std::nth_element has permuted it) this
file adds in NumPy's order. The normal equations are solved by np.linalg.solve (LU with partial
pivoting) where the node calls Eigen's pivoted ldlt(); the two agree to rounding times
cond(AᵀA + εI), which lift() returns per feature with the other quantities the test conditions are
stated on: |det H_uv| / ‖H_uv‖_F², the window and fit counts, the row kinds, and kappa_app before
the w_ma factor. The depth window's count of a `nearest` sample is 1 or 0 (the node keeps no zs
there). cfg is any object with the VisualFeatureConfig fields."""

from __future__ import annotations

import math

import numpy as np

K_EPS = 1e-12  # kEps (:34)
MAD_NORMAL_SCALE = 1.4826
FLOAT_KEYS = ("depth_Lambda_c", "depth_theta_c", "weight", "kappa_app", "mu_app", "xyz", "cov_xyz",
              "depth_sigma_c_sq", "lam_min", "K")
FIT_KEYS = ("kappa_app", "mu_app", "cov_xyz", "lam_min", "K")  # what depends on the solve


def round_half_away(x):
    """std::round: halves away from zero (np.round goes to even). x - trunc(x) is exact."""
    x = np.asarray(x, np.float64)
    t = np.trunc(x)
    return t + np.sign(x) * (np.abs(x - t) >= 0.5)


def sigmoid(x):  # safe_sigmoid (:37-44)
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(x))
    return np.where(x >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))


def window_offsets(r):
    """(dx, dy) of a (2r+1)^2 window in the order the node visits it: rows, then columns (:266-267, :410-411)."""
    return [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]


def hex_offsets(radius):
    """:303-312: the centre and round(r cos(k π/3)), round(r sin(k π/3)), k = 0..5, r = max(1, hex_radius)."""
    r = max(1, int(radius))
    out = [(0, 0)]
    for k in range(6):
        ang = float(k) * math.pi / 3.0
        out.append((int(round_half_away(r * math.cos(ang))), int(round_half_away(r * math.sin(ang)))))
    return out


def _gather(depth, x, y, ok, offsets, scale):
    """depth_to_meters of the pixels (x + dx, y + dy) of the rows with ok, and which of them the node
    keeps: inside the image, finite and positive (:268-271, :316-323, :414-418)."""
    H, W = depth.shape
    dx = np.array([o[0] for o in offsets], np.int64)
    dy = np.array([o[1] for o in offsets], np.int64)
    xi, yi = x[:, None] + dx[None], y[:, None] + dy[None]
    inside = ok[:, None] & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
    z = np.zeros(xi.shape, np.float64)
    z[inside] = depth[yi[inside], xi[inside]].astype(np.float64) * float(scale)
    with np.errstate(invalid="ignore"):
        keep = inside & np.isfinite(z) & (z > 0.0)
    return np.where(keep, z, 0.0), keep, xi, yi


def _rank_half(vals, keep):
    """The element of rank size/2 of each row's kept values (std::nth_element at begin + size / 2;
    :279-280, :332-333, :340-341); NaN for an empty row."""
    n = keep.sum(axis=1)
    s = np.sort(np.where(keep, vals, np.inf), axis=1)
    out = s[np.arange(vals.shape[0]), np.minimum(n // 2, vals.shape[1] - 1)]
    return np.where(n > 0, out, np.nan)


def depth_sigma(z_m, cfg):  # :216-226
    z = np.abs(z_m)
    if cfg.depth_model == "linear":
        return cfg.depth_sigma0 + cfg.depth_sigma_slope * z
    if cfg.depth_model == "quadratic":
        return cfg.depth_sigma0 + cfg.depth_sigma_slope * (z * z)
    raise ValueError("Unknown depth_model: " + str(cfg.depth_model))


def lift(depth, rgb, keypoints, intrinsics, cfg):
    """keypoints (M, 3) = (u, v, response); depth (H, W) float32; rgb (H, W, 3) uint8 or None.
    Returns a dict with the CameraFeatures arrays, the aux columns under their names, and `cond`."""
    depth = np.asarray(depth)
    assert depth.dtype == np.float32 and depth.ndim == 2
    H, W = depth.shape
    kp = np.asarray(keypoints, np.float64).reshape(-1, 3)
    M = kp.shape[0]
    u, v, resp = kp[:, 0], kp[:, 1], kp[:, 2]
    fx, fy, cx, cy = (float(t) for t in intrinsics)

    # ---- depth_sample (:228-297), depth_sample_hex (:299-348)
    x, y = round_half_away(u).astype(np.int64), round_half_away(v).astype(np.int64)
    in_image = (x >= 0) & (y >= 0) & (x < W) & (y < H)
    mode = cfg.depth_sample_mode
    if mode == "nearest":
        offsets = [(0, 0)]
    elif mode == "median3":
        offsets = window_offsets(1)
    elif mode == "median5":
        offsets = window_offsets(2)
    elif mode == "hex":
        offsets = hex_offsets(cfg.hex_radius)
    else:
        raise ValueError("Unknown depth_sample_mode: " + str(mode))
    zs, keep, _, _ = _gather(depth, x, y, in_image, offsets, cfg.depth_scale)
    n_win = keep.sum(axis=1)
    z_var = np.full(M, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == "nearest":
            z_valid = n_win == 1
            z_m = zs[:, 0].copy()
        elif mode == "hex":
            z_valid = n_win >= 4                                        # :327
            z_m = _rank_half(zs, keep)
            mad = _rank_half(np.abs(zs - z_m[:, None]), keep)           # :335-341
            z_var = np.where(z_valid, (MAD_NORMAL_SCALE * mad) ** 2, np.nan)
        else:
            z_valid = n_win >= 1
            z_m = _rank_half(zs, keep)
            mean = zs.sum(axis=1) / n_win                               # :282-292 (zs is 0 outside keep)
            var = np.where(keep, (zs - mean[:, None]) ** 2, 0.0).sum(axis=1) / n_win
            z_var = np.where(n_win >= 4, var, np.nan)
    z_m = np.where(z_valid, z_m, np.nan)
    z_var = np.where(z_valid & np.isfinite(z_var), z_var, np.nan)       # validate_depth (:184-194)

    # ---- the weight (:554-556) from depth_weight (:196-205) and response_weight (:207-214)
    a = cfg.depth_validity_slope
    with np.errstate(over="ignore", invalid="ignore"):
        w_lo = 1.0 / (1.0 + np.exp(-a * (z_m - cfg.min_depth_m)))
        w_hi = 1.0 / (1.0 + np.exp(+a * (z_m - cfg.max_depth_m)))
        w_depth = np.where(z_valid, np.clip(w_lo * w_hi, 0.0, 1.0), 0.0)
        w_resp = np.where(resp <= 0.0, 0.0, resp / (resp + cfg.response_soft_scale))
    weight = np.clip(w_depth * w_resp, 0.0, 1.0)

    # ---- var_z_eff (:563-572) and student_t_effective_var (:350-369)
    sig_sq = depth_sigma(z_m, cfg) ** 2                                 # NaN without a valid depth
    from_window = z_valid & np.isfinite(z_var)
    with np.errstate(invalid="ignore", divide="ignore"):
        base_var = np.where(from_window, np.where(z_var < sig_sq, sig_sq, z_var), np.nan)   # std::max(z_var, σ²)
        student = from_window & (n_win >= 2) & np.isfinite(base_var) & (base_var > 0.0)
        q = np.where(keep, (zs - z_m[:, None]) ** 2, 0.0).sum(axis=1)
        q = q / (n_win * np.maximum(base_var, K_EPS) + K_EPS)
        w_t = (cfg.student_t_nu + 1.0) / (cfg.student_t_nu + q)
        w_t = np.where(w_t < cfg.student_t_w_min, cfg.student_t_w_min, w_t)
        var_eff = np.where(student, base_var / w_t, base_var)
    var_eff = np.where(from_window, var_eff, np.where(z_valid, sig_sq, np.nan))
    var_eff = np.where(z_valid & ~np.isfinite(var_eff), sig_sq, var_eff)

    # ---- quadratic_fit (:401-491)
    rq = max(1, int(cfg.quad_fit_radius))
    qz, qkeep, xi, yi = _gather(depth, x, y, z_valid, window_offsets(rq), cfg.depth_scale)
    n_fit = qkeep.sum(axis=1)
    fit = z_valid & (n_fit >= int(cfg.quad_fit_min_points))
    normal = np.zeros((M, 3))
    K_curv, lam_min, det_ratio, cond = np.zeros(M), np.zeros(M), np.full(M, np.nan), np.full(M, np.nan)
    beta = np.full((M, 6), np.nan)
    if fit.any():
        f = np.nonzero(fit)[0]
        ut, vt = xi[f] - u[f, None], yi[f] - v[f, None]                 # relative to the unrounded keypoint
        A = np.stack([ut * ut, ut * vt, vt * vt, ut, vt, np.ones_like(ut)], axis=2) * qkeep[f][:, :, None]
        AtA = np.einsum("mpi,mpj->mij", A, A) + cfg.quad_fit_lstsq_eps * np.eye(6)[None]    # :442-443
        Atb = np.einsum("mpi,mp->mi", A, qz[f])
        bt = np.linalg.solve(AtA, Atb[:, :, None])[:, :, 0]
        beta[f] = bt
        cond[f] = np.linalg.cond(AtA)
        zc = np.where(z_m[f] < 1e-6, 1e-6, z_m[f])                      # std::max(z_hat, 1e-6)
        sx, sy = fx / zc, fy / zc
        zu, zv = sx * bt[:, 3], sy * bt[:, 4]
        h00, h01, h11 = sx * sx * (2.0 * bt[:, 0]), sx * sy * bt[:, 1], sy * sy * (2.0 * bt[:, 2])
        det_H = h00 * h11 - h01 * h01
        denom = 1.0 + (zu * zu + zv * zv)
        with np.errstate(invalid="ignore", divide="ignore"):
            K_curv[f] = np.where(denom > 0.0, det_H / (denom * denom), 0.0)
            det_ratio[f] = np.abs(det_H) / (h00 * h00 + 2.0 * h01 * h01 + h11 * h11)
        Huv = np.stack([np.stack([h00, h01], axis=1), np.stack([h01, h11], axis=1)], axis=1)
        lam_min[f] = np.linalg.eigvalsh(Huv)[:, 0]
        nrm = np.stack([-zu, -zv, np.ones_like(zu)], axis=1)
        nn = np.linalg.norm(nrm, axis=1)
        normal[f] = np.where(nn[:, None] > 0.0, nrm / nn[:, None], nrm)

    # ---- the assembly (:574-634)
    w_ma = np.where(fit, sigmoid(cfg.ma_tau * lam_min), 0.0)
    xyz = np.zeros((M, 3))
    cov = np.zeros((M, 3, 3))
    cov[:] = np.eye(3) * cfg.invalid_cov_inflate
    if z_valid.any():
        g = np.nonzero(z_valid)[0]
        zz, du, dv = z_m[g], u[g] - cx, v[g] - cy
        xyz[g] = np.stack([du * zz / fx, dv * zz / fy, zz], axis=1)     # :371-376
        var_use = np.where(var_eff[g] < sig_sq[g], sig_sq[g], var_eff[g])                   # :579
        vu = vv = max(cfg.pixel_sigma * cfg.pixel_sigma, 0.0)
        vz = np.where(var_use < 0.0, 0.0, var_use)
        c = np.zeros((g.shape[0], 3, 3))                                # :378-399
        c[:, 0, 0] = (zz * zz * vu + du * du * vz + vu * vz) / (fx * fx)
        c[:, 1, 1] = (zz * zz * vv + dv * dv * vz + vv * vz) / (fy * fy)
        c[:, 2, 2] = vz
        c[:, 0, 1] = c[:, 1, 0] = (du * dv * vz) / (fx * fy)
        c[:, 0, 2] = c[:, 2, 0] = (du * vz) / fx
        c[:, 1, 2] = c[:, 2, 1] = (dv * vz) / fy
        c += (np.where(fit[g], (1.0 - w_ma[g]) * cfg.ma_delta_inflate, 0.0))[:, None, None] * np.eye(3)[None]
        cov[g] = c
    with np.errstate(invalid="ignore", divide="ignore"):
        rel_noise = np.where(z_valid & np.isfinite(var_eff), np.sqrt(var_eff) / (z_m + K_EPS), 1.0)     # :592-594
        rho = 1.0 / (rel_noise + K_EPS)
        kappa_raw = cfg.kappa0 + cfg.kappa_alpha * np.sqrt(np.abs(K_curv)) * rho
        kappa_clamped = np.where(fit, np.maximum(cfg.kappa_min, np.minimum(cfg.kappa_max, kappa_raw)), 0.0)
        kappa_app = kappa_clamped * w_ma
        has_depth_c = z_valid & np.isfinite(var_eff) & (var_eff > 0.0)                                  # :605
        sigma_c_sq = np.where(has_depth_c, var_eff, np.nan)
        Lambda_c = np.where(has_depth_c, 1.0 / var_eff, 0.0)
        theta_c = np.where(has_depth_c, Lambda_c * z_m, 0.0)
    color = np.zeros((M, 3))
    if rgb is not None:                                                 # :611-616
        rgb = np.asarray(rgb)
        assert rgb.dtype == np.uint8 and rgb.shape == (H, W, 3)
        ix = round_half_away(np.clip(u, 0.0, float(W - 1))).astype(np.int64)
        iy = round_half_away(np.clip(v, 0.0, float(H - 1))).astype(np.int64)
        color = rgb[iy, ix].astype(np.float64) / 255.0

    # ---- backend_node.py:1600-1601, :1616-1620
    bad_cov = ~np.isfinite(cov).all(axis=(1, 2))
    cov[bad_cov] = np.eye(3) * 1e6
    mu_norm = np.linalg.norm(normal, axis=1)
    has_mu = fit & np.isfinite(normal).all(axis=1) & (mu_norm > 0.0)
    mu_app = np.where(has_mu[:, None], normal / (mu_norm[:, None] + 1e-12), 0.0)

    return dict(
        u=u.copy(), v=v.copy(), depth_Lambda_c=Lambda_c, depth_theta_c=theta_c, weight=weight, kappa_app=kappa_app,
        mu_app=mu_app, has_mu_app=has_mu, color=color, has_color=np.full(M, rgb is not None), xyz=xyz, cov_xyz=cov,
        depth_sigma_c_sq=sigma_c_sq, z_m=z_m, n_window=n_win.astype(np.float64), n_fit=n_fit.astype(np.float64),
        lam_min=lam_min, K=K_curv,
        cond=dict(cond=cond, det_ratio=det_ratio, n_window=n_win, n_fit=n_fit, in_image=in_image, z_valid=z_valid,
                  fit=fit, from_window=from_window & (z_var > np.where(np.isfinite(sig_sq), sig_sq, np.inf)),
                  kappa_clamped=kappa_clamped, w_ma=w_ma, beta=beta, x=x, y=y))


def aux_columns(out):
    """The (M, GC_CAMFEAT_AUX) array of a lift() result."""
    return np.stack([out[k] for k in ("depth_sigma_c_sq", "z_m", "n_window", "n_fit", "lam_min", "K")], axis=1)


def determined(cond, cond_max=1e6, det_min=1e-4):
    """The fitted rows whose solve and whose det H_uv the inputs pin: cond(AᵀA + εI) < cond_max and
    |det H_uv| / ‖H_uv‖_F² >= det_min."""
    with np.errstate(invalid="ignore"):
        return cond["fit"] & (cond["cond"] < cond_max) & (cond["det_ratio"] >= det_min)
