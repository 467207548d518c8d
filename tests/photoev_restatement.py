"""TEST INFRASTRUCTURE — a NumPy restatement of the photometric pose evidence ("Photometric
pose evidence"), in plain loops, built on the camera view's restatement (camrender_restatement.py) and the
depth evidence's (depthev_restatement.py: the pose conventions and the splat tangents): the luminance of
every splat and its six pose tangents (the tangent of the vMF shading towards the camera), carried forward
through the compositing loop of every pixel, and the Gaussian evidence (L6, h6) of an observed luminance
image. tests/test_photo_evidence.py holds this file to central differences of camrender_restatement and to
closed forms; the GPU tests hold the device to this file."""

import numpy as np

import camrender_restatement as CS
import depthev_restatement as DS

GREY = (4899.0 / 16384.0, 9617.0 / 16384.0, 1868.0 / 16384.0)
PCFG = dict(sigma=0.05, weights=GREY, robust_nu=None, eps_lift=1e-9)
PARTS = DS.PARTS


def pconfig(**kw):
    c = dict(PCFG)
    c.update(kw)
    return c


def luminance(c, w):
    """y = (w_r r + w_g g) + w_b b over the last axis."""
    c = np.asarray(c, np.float64)
    return (w[0] * c[..., 0] + w[1] * c[..., 1]) + w[2] * c[..., 2]


def image_luminance(rgb8, w=GREY):
    """An (H, W, 3) uint8 image as the float32 luminance the evidence observes."""
    return (luminance(np.asarray(rgb8, np.uint8).astype(np.float64), w) / 255.0).astype(np.float32)


def shading_tangent(vd, dc, eta, eps=1e-12):
    """The tangents ds (6) of camrender_restatement.vmf_shading at the view direction vd (not normalised)
    for the tangents dc (6, 3) of vd; eta (B, 3). The eps terms are differentiated as written."""
    vd = np.asarray(vd, np.float64)
    n = np.sqrt(np.sum(vd ** 2))
    nv = n + eps
    v = vd / nv
    B = eta.shape[0]
    ds, ksum = np.zeros(6), 0.0
    for k in range(6):
        dv = dc[k] / nv - vd * (vd @ dc[k]) / (n * nv * nv)
        for b in range(B):
            kap = np.sqrt(np.sum(eta[b] ** 2))
            m = eta[b] / (kap + eps)
            ds[k] += np.exp(kap * (m @ v - 1.0)) * kap * (m @ dv) / B
    for b in range(B):
        ksum += np.sqrt(np.sum(eta[b] ** 2))
    return ds / (1.0 + ksum / B)


def centre_tangents(T_cw, t_wb):
    """The six tangents (6, 3) of the camera centre c = -R^T t: e_k for dt_k, e_k x (c - t_wb) for dtheta_k."""
    c = -T_cw[:3, :3].T @ T_cw[:3, 3]
    return c, np.concatenate([np.eye(3), np.stack([np.cross(e, c - t_wb) for e in np.eye(3)])])


def shade_tangents(batch, T_cw, t_wb, cfg, s, w):
    """lum (n): the luminance of prep's colour rows; dlum (n, 6) = (w . color) ds_k, zero where the row is
    not valid or the view is not shaded. s: prep's outputs for this view."""
    mu, eta = np.asarray(batch["mu_world"], np.float64), np.asarray(batch["eta"], np.float64)
    col = np.asarray(batch["color"], np.float64)
    n = mu.shape[0]
    lum, dlum = np.zeros(n), np.zeros((n, 6))
    c, dc = centre_tangents(np.asarray(T_cw, np.float64), np.asarray(t_wb, np.float64))
    for i in range(n):
        if not s["valid"][i]:
            continue
        lum[i] = luminance(s["colors"][i], w)
        if cfg["shade"]:
            dlum[i] = luminance(col[i], w) * shading_tangent(c - mu[i], dc, eta[i])
    return lum, dlum


def composite_pixel_jvp(px, py, lst, s, tan, lum, dlum, cfg, cond=None):
    """One pixel over one list, in list order with composite_pixel's branches: (T, Y, dT (6), dY (6))."""
    dm, _, dS = tan
    T, Y, dT, dY = 1.0, 0.0, np.zeros(6), np.zeros(6)
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
        y = lum[i]
        flat = raw > cfg["alpha_max"] or q < 0.0
        if cond is not None and raw > cfg["alpha_max"]:
            cond["alpha_capped"] += 1
        g = Si @ d
        for k in range(6):
            dq = -2.0 * (g @ dm[i, k]) + (dS[i, k, 0] * d[0] * d[0] + 2.0 * dS[i, k, 1] * d[0] * d[1]
                                          + dS[i, k, 2] * d[1] * d[1])
            da = 0.0 if flat else -0.5 * a * dq
            dY[k] += dT[k] * a * y + T * da * y + T * a * dlum[i, k]
            dT[k] = dT[k] * (1.0 - a) - T * da
        Y += T * a * y
        T = T * (1.0 - a)
        if T < cfg["t_stop"]:
            if cond is not None:
                cond["stopped"] += 1
            break
    return T, Y, dT, dY


def evidence_one(batch, K, T_wb, lum_obs, H, W, cfg, pcfg, R_bc=None, t_bc=None):
    """One pose. lum_obs (H, W): float32 values, NaN or an infinity for a hole. Returns the render
    (camrender_restatement.render's dict for the one view), lum, dlum, lum_render = Y / A (0 where A <= eps),
    J (H, W, 6; zero where A <= eps), used, residual, weight, L6, h6, cost, n_used, sum_cov, sum_w, L_pose
    (22, 22), h_pose (22), parts (46) and `cond` (render's conditions and skipped / stopped / alpha_capped
    counts of the tangent loop)."""
    T_wb = np.asarray(T_wb, np.float64)
    T_cw = CS.camera_from_world(T_wb, R_bc, t_bc)
    out, conds = CS.render(batch, [K], [T_cw], H, W, cfg)
    s = {k: (out[k] if k == "alphas" else out[k][0]) for k in out}
    tan = DS.splat_tangents(batch, K, T_cw, T_wb[:3, 3], H, W, cfg, s)
    w3 = pcfg["weights"]
    lum, dlum = shade_tangents(batch, T_cw, T_wb[:3, 3], cfg, s, w3)
    ts = cfg["tile_size"]
    tiles_x = W // ts
    obs = np.asarray(lum_obs, np.float64)
    assert obs.shape == (H, W), obs.shape
    J, used = np.zeros((H, W, 6)), np.zeros((H, W), bool)
    res, wgt, yr = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    L6, h6 = np.zeros((6, 6)), np.zeros(6)
    cost = sum_cov = sum_w = 0.0
    nu, sg = pcfg["robust_nu"], pcfg["sigma"]
    cond = dict(conds[0], skipped=0, stopped=0, alpha_capped=0)
    for row in range(H):
        for col in range(W):
            t = (row // ts) * tiles_x + col // ts
            T, Y, dT, dY = composite_pixel_jvp(col + 0.5, row + 0.5, s["tile_indices"][t, :s["tile_counts"][t]], s, tan,
                                               lum, dlum, cfg, cond)
            A = s["alpha"][row, col]
            assert A == 1.0 - T
            if not A > cfg["eps"]:
                continue
            J[row, col] = (dY * A + Y * dT) / (A * A)
            yr[row, col] = Y / A
            o = obs[row, col]
            if not np.isfinite(o):
                continue
            used[row, col] = True
            r = Y / A - o
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
    L_pose[:6, :6] = L6 + pcfg["eps_lift"] * np.eye(6)
    h_pose[:6] = h6
    parts = np.concatenate([L6.reshape(-1), h6, [cost, float(n_used), sum_cov, sum_w]])
    return dict(render=s, lum=lum, dlum=dlum, lum_render=yr, J=J, used=used, residual=res, weight=wgt, L6=L6, h6=h6, cost=cost,
                n_used=n_used, sum_cov=sum_cov, sum_w=sum_w, L_pose=L_pose, h_pose=h_pose, parts=parts, cond=cond)


def evidence(batch, K, T_wbs, lum_obs, H, W, cfg, pcfg, R_bc=None, t_bc=None):
    """Every pose: evidence_one's arrays stacked (the device's shapes) and the per-pose conditions."""
    per = [evidence_one(batch, K, T, lum_obs, H, W, cfg, pcfg, R_bc, t_bc) for T in T_wbs]
    keys = ("lum", "dlum", "lum_render", "J", "used", "residual", "weight", "L6", "h6", "L_pose", "h_pose", "parts")
    out = {k: np.stack([p[k] for p in per]) for k in keys}
    out["alpha"] = np.stack([p["render"]["alpha"] for p in per])
    out["n_contrib"] = np.stack([p["render"]["n_contrib"] for p in per])
    out["valid"] = np.stack([p["render"]["valid"] for p in per])
    for k in ("cost", "n_used", "sum_cov", "sum_w"):
        out[k] = np.array([p[k] for p in per])
    return out, [p["cond"] for p in per]
