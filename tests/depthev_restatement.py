"""TEST INFRASTRUCTURE — a NumPy restatement of the depth pose evidence ("Depth pose
evidence"), in plain loops, built on the camera view's restatement (camrender_restatement.py): the six
pose tangents of every splat, carried forward through the compositing loop of every pixel, and the
Gaussian evidence (L6, h6) of an observed depth image. tests/test_depth_evidence.py holds this file to
central differences of camrender_restatement.render and to closed forms; the GPU tests hold the device
to this file.

The tangent convention is visual_pose_evidence.py's (r = map - (R m + t), d/dt = -I, :89-99;
R_delta = R_scatter R_pred^T, :234-238): delta = [dt, dtheta] with t_wb' = t_wb + dt and
R_wb' = Exp(dtheta) R_wb."""

import numpy as np

import camrender_restatement as CS

ECFG = dict(depth_model="linear", depth_sigma0=0.01, depth_sigma_slope=0.01, min_depth_m=0.05, max_depth_m=80.0,
            robust_nu=None, eps_lift=1e-9)
PARTS = 46


def econfig(**kw):
    c = dict(ECFG)
    c.update(kw)
    return c


def hat(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def so3_exp(w):
    """Rodrigues."""
    w = np.asarray(w, np.float64)
    th = np.sqrt(w @ w)
    K = hat(w)
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / th ** 2) * (K @ K)


def pose_matrix(pose6):
    """T_wb (4, 4) of a pose [t, rotvec]."""
    p = np.asarray(pose6, np.float64)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = so3_exp(p[3:]), p[:3]
    return T


def perturbed(T_wb, delta):
    """T_wb moved by delta = [dt, dtheta]: t + dt, Exp(dtheta) R."""
    d = np.asarray(delta, np.float64)
    T = np.array(T_wb, np.float64)
    T[:3, :3] = so3_exp(d[3:]) @ T[:3, :3]
    T[:3, 3] = T[:3, 3] + d[:3]
    return T


def splat_tangents(batch, K, T_cw, t_wb, H, W, cfg, s):
    """The six tangents of prep's means_px (n, 6, 2), depths (n, 6) and Sigmas_inv (n, 6, 3: the entries
    00, 01, 11); zero where the row is not valid. s: prep's outputs for this view."""
    mu, Sig = np.asarray(batch["mu_world"], np.float64), np.asarray(batch["Sigma_world"], np.float64)
    n = mu.shape[0]
    fx, fy, cx, cy = K
    R, t = T_cw[:3, :3], T_cw[:3, 3]
    limx, limy = 1.3 * max(cx, W - cx) / fx, 1.3 * max(cy, H - cy) / fy
    dm, dz_, dS = np.zeros((n, 6, 2)), np.zeros((n, 6)), np.zeros((n, 6, 3))
    for i in range(n):
        if not s["valid"][i]:
            continue
        x, y, z = R @ mu[i] + t
        ux, uy = x / z, y / z
        tx, ty = np.clip(ux, -limx, limx) * z, np.clip(uy, -limy, limy) * z
        J = np.array([[fx / z, 0.0, -fx * tx / z ** 2], [0.0, fy / z, -fy * ty / z ** 2]])
        M = J @ R
        Si = s["Sigmas_inv"][i]
        for k in range(6):
            e = np.zeros(3)
            e[k % 3] = 1.0
            if k < 3:
                dp, dR = -R @ e, np.zeros((3, 3))
            else:
                dp, dR = R @ hat(mu[i] - t_wb) @ e, -R @ hat(e)
            dx, dy, dz = dp
            dm[i, k] = [fx * (dx / z - x * dz / z ** 2), fy * (dy / z - y * dz / z ** 2)]
            dz_[i, k] = dz
            dtx = dx if abs(ux) <= limx else np.sign(ux) * limx * dz
            dty = dy if abs(uy) <= limy else np.sign(uy) * limy * dz
            dJ = np.array([[-fx * dz / z ** 2, 0.0, -fx * (dtx / z ** 2 - 2.0 * tx * dz / z ** 3)],
                           [0.0, -fy * dz / z ** 2, -fy * (dty / z ** 2 - 2.0 * ty * dz / z ** 3)]])
            dM = dJ @ R + J @ dR
            dSp = dM @ Sig[i] @ M.T + M @ Sig[i] @ dM.T
            dSp = 0.5 * (dSp + dSp.T)
            dSi = -Si @ dSp @ Si
            dS[i, k] = [dSi[0, 0], 0.5 * (dSi[0, 1] + dSi[1, 0]), dSi[1, 1]]
    return dm, dz_, dS


def composite_pixel_jvp(px, py, lst, s, tan, cfg, cond=None):
    """One pixel over one list, in list order with composite_pixel's branches: (T, D, dT (6), dD (6))."""
    dm, dz_, dS = tan
    T, D, dT, dD = 1.0, 0.0, np.zeros(6), np.zeros(6)
    for i in lst:
        d = np.array([px, py]) - s["means_px"][i]
        Si = s["Sigmas_inv"][i]
        q = (d[0] * Si[0, 0] + d[1] * Si[1, 0]) * d[0] + (d[0] * Si[0, 1] + d[1] * Si[1, 1]) * d[1]
        raw = s["alphas"][i] * np.exp(-0.5 * max(q, 0.0))
        a = min(cfg["alpha_max"], raw)
        if a < cfg["alpha_skip"]:
            if cond is not None:
                cond["skipped"] += 1
            continue
        z = s["depths"][i]
        flat = raw > cfg["alpha_max"] or q < 0.0
        if cond is not None and raw > cfg["alpha_max"]:
            cond["alpha_capped"] += 1
        g = Si @ d
        for k in range(6):
            dq = -2.0 * (g @ dm[i, k]) + (dS[i, k, 0] * d[0] * d[0] + 2.0 * dS[i, k, 1] * d[0] * d[1]
                                          + dS[i, k, 2] * d[1] * d[1])
            da = 0.0 if flat else -0.5 * a * dq
            dD[k] += dT[k] * a * z + T * da * z + T * a * dz_[i, k]
            dT[k] = dT[k] * (1.0 - a) - T * da
        D += T * a * z
        T = T * (1.0 - a)
        if T < cfg["t_stop"]:
            if cond is not None:
                cond["stopped"] += 1
            break
    return T, D, dT, dD


def sigma_of(d, ecfg):
    if ecfg["depth_model"] == "quadratic":
        return ecfg["depth_sigma0"] + ecfg["depth_sigma_slope"] * d * d
    return ecfg["depth_sigma0"] + ecfg["depth_sigma_slope"] * d


def evidence_one(batch, K, T_wb, depth_obs, H, W, cfg, ecfg, R_bc=None, t_bc=None):
    """One pose. Returns the render (camrender_restatement.render's dict for the one view), the tangent
    arrays, J (H, W, 6; zero where A <= eps), used, residual, weight (H, W), L6, h6, cost, n_used, sum_cov,
    sum_w, L_pose (22, 22), h_pose (22), parts (46) and `cond` (render's conditions and skipped / stopped /
    alpha_capped counts of the tangent loop)."""
    T_wb = np.asarray(T_wb, np.float64)
    T_cw = CS.camera_from_world(T_wb, R_bc, t_bc)
    out, conds = CS.render(batch, [K], [T_cw], H, W, cfg)
    s = {k: (out[k] if k == "alphas" else out[k][0]) for k in out}
    tan = splat_tangents(batch, K, T_cw, T_wb[:3, 3], H, W, cfg, s)
    ts = cfg["tile_size"]
    tiles_x = W // ts
    cond = dict(conds[0], skipped=0, stopped=0, alpha_capped=0)
    obs = np.asarray(depth_obs, np.float64)  # the cases hold float32 values, as the device takes them
    assert obs.shape == (H, W), obs.shape
    J, used = np.zeros((H, W, 6)), np.zeros((H, W), bool)
    res, wgt = np.zeros((H, W)), np.zeros((H, W))
    L6, h6 = np.zeros((6, 6)), np.zeros(6)
    cost = sum_cov = sum_w = 0.0
    nu = ecfg["robust_nu"]
    for row in range(H):
        for col in range(W):
            t = (row // ts) * tiles_x + col // ts
            T, D, dT, dD = composite_pixel_jvp(col + 0.5, row + 0.5, s["tile_indices"][t, :s["tile_counts"][t]], s, tan,
                                               cfg, cond)
            A = s["alpha"][row, col]
            assert A == 1.0 - T
            if A > cfg["eps"]:
                J[row, col] = (dD * A + D * dT) / (A * A)
            o = obs[row, col]
            if not (np.isfinite(o) and ecfg["min_depth_m"] < o < ecfg["max_depth_m"] and A > cfg["eps"]):
                continue
            used[row, col] = True
            r = s["depth"][row, col] - o
            sg = sigma_of(o, ecfg)
            u = 1.0 if nu is None else (nu + 1.0) / (nu + (r / sg) ** 2)
            w = A * u / (sg * sg)
            res[row, col], wgt[row, col] = r, w
            L6 += w * np.outer(J[row, col], J[row, col])
            h6 -= w * J[row, col] * r
            cost += w * r * r
            sum_cov += A
            sum_w += w
    n_used = int(used.sum())
    L_pose, h_pose = np.zeros((22, 22)), np.zeros(22)
    L_pose[:6, :6] = L6 + ecfg["eps_lift"] * np.eye(6)
    h_pose[:6] = h6
    parts = np.concatenate([L6.reshape(-1), h6, [cost, float(n_used), sum_cov, sum_w]])
    return dict(render=s, dmeans_px=tan[0], ddepths=tan[1], dSigmas_inv=tan[2], J=J, used=used, residual=res, weight=wgt,
                L6=L6, h6=h6, cost=cost, n_used=n_used, sum_cov=sum_cov, sum_w=sum_w, L_pose=L_pose, h_pose=h_pose,
                parts=parts, cond=cond)


def evidence(batch, K, T_wbs, depth_obs, H, W, cfg, ecfg, R_bc=None, t_bc=None):
    """Every pose: evidence_one's arrays stacked (the device's shapes) and the per-pose conditions."""
    per = [evidence_one(batch, K, T, depth_obs, H, W, cfg, ecfg, R_bc, t_bc) for T in T_wbs]
    keys = ("dmeans_px", "ddepths", "dSigmas_inv", "J", "used", "residual", "weight", "L6", "h6", "L_pose", "h_pose",
            "parts")
    out = {k: np.stack([p[k] for p in per]) for k in keys}
    out["depth"] = np.stack([p["render"]["depth"] for p in per])
    out["alpha"] = np.stack([p["render"]["alpha"] for p in per])
    out["n_contrib"] = np.stack([p["render"]["n_contrib"] for p in per])
    for k in ("cost", "n_used", "sum_cov", "sum_w"):
        out[k] = np.array([p[k] for p in per])
    return out, [p["cond"] for p in per]
