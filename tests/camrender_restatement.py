"""TEST INFRASTRUCTURE — a NumPy restatement of the camera view ("Camera view"), in plain
loops, with what the conditions of tests/test_camera_render.py read. What the reference's viewer does
around jaxsplat.render_v2 (tools/view_splat_jaxsplat.py:103-114: T_cw = inv(T_wb), alpha =
clip(w / w_max, 0.01, 1), eta = kappa d) is followed to the letter; the raster is the standard 3D
Gaussian splatting forward pass as the build defines it. tests/test_camera_render.py holds this file to
closed forms; the GPU tests hold the device to this file."""

import numpy as np

CFG = dict(tile_size=16, max_splats_per_tile=256, near=0.2, far=100.0, lowpass_px2=0.3, radius_sigma=3.0,
           alpha_floor=0.01, alpha_max=0.99, alpha_skip=1.0 / 255.0, t_stop=1e-4, background=(0.0, 0.0, 0.0),
           shade=True, eps=1e-12)


def config(**kw):
    c = dict(CFG)
    c.update(kw)
    return c


def camera_from_world(T_wb, R_bc=None, t_bc=None):
    """T_cw = inv(T_wb T_bc) (view_splat_jaxsplat.py:103 with the camera at the body by default)."""
    T_bc = np.eye(4)
    if R_bc is not None:
        T_bc[:3, :3] = R_bc
    if t_bc is not None:
        T_bc[:3, 3] = t_bc
    return np.linalg.inv(np.asarray(T_wb, np.float64) @ T_bc)


def vmf_shading(v, eta, eps=1e-12):
    """rendering.py:135-159 with uniform lobe weights and no intensity, one row: v (3,), eta (B, 3)."""
    v = np.asarray(v, np.float64) / (np.sqrt(np.sum(np.asarray(v, np.float64) ** 2)) + eps)
    B = eta.shape[0]
    s, ksum = 0.0, 0.0
    for b in range(B):
        kap = np.sqrt(np.sum(eta[b] ** 2))
        mu = eta[b] / (kap + eps)
        s += np.exp(kap * (mu @ v - 1.0)) / B
        ksum += kap
    return s / (1.0 + ksum / B)


def project(p, K):
    """The pinhole: (fx x / z + cx, fy y / z + cy)."""
    fx, fy, cx, cy = K
    return np.array([fx * p[0] / p[2] + cx, fy * p[1] / p[2] + cy])


def alphas_from_mass(mass, alpha_floor):
    """view_splat_jaxsplat.py:108-111: mass / m_max clipped to [alpha_floor, 1]; m_max = 1 unless positive."""
    mass = np.asarray(mass, np.float64)
    m_max = float(np.max(mass)) if mass.size and np.max(mass) > 0 else 1.0
    return np.clip(mass / m_max, alpha_floor, 1.0)


def prep(batch, K, T_cw, H, W, cfg):
    """One view's 2D splats. batch: mu_world (n, 3), Sigma_world (n, 3, 3), eta (n, B, 3), mass (n),
    color (n, 3). Returns the arrays and `cond`: the smallest near / far margin, the largest condition
    number of Sigma_px, the number of primitives at the tangent clamp."""
    mu, Sig = np.asarray(batch["mu_world"], np.float64), np.asarray(batch["Sigma_world"], np.float64)
    n = mu.shape[0]
    fx, fy, cx, cy = K
    R, t = T_cw[:3, :3], T_cw[:3, 3]
    centre = -R.T @ t
    out = dict(means_px=np.zeros((n, 2)), Sigmas_inv=np.zeros((n, 2, 2)), depths=np.full(n, np.inf), radii=np.zeros(n),
               alphas=alphas_from_mass(batch["mass"], cfg["alpha_floor"]), colors=np.zeros((n, 3)),
               valid=np.zeros(n, np.uint8), Sigmas_px=np.zeros((n, 2, 2)))
    cond = dict(z_margin=np.inf, condition=0.0, clamped=0)
    limx, limy = 1.3 * max(cx, W - cx) / fx, 1.3 * max(cy, H - cy) / fy
    for i in range(n):
        with np.errstate(invalid="ignore", over="ignore"):
            p = R @ mu[i] + t
        if not (np.isfinite(p).all() and np.isfinite(Sig[i]).all()):
            continue
        x, y, z = p
        cond["z_margin"] = min(cond["z_margin"], abs(z - cfg["near"]), abs(z - cfg["far"]))
        if not (cfg["near"] < z < cfg["far"]):
            continue
        tx, ty = np.clip(x / z, -limx, limx) * z, np.clip(y / z, -limy, limy) * z
        cond["clamped"] += int(abs(x / z) > limx or abs(y / z) > limy)
        J = np.array([[fx / z, 0.0, -fx * tx / z ** 2], [0.0, fy / z, -fy * ty / z ** 2]])
        M = J @ R
        S = M @ Sig[i] @ M.T
        S = 0.5 * (S + S.T) + cfg["lowpass_px2"] * np.eye(2)
        a, b, d = S[0, 0], S[1, 0], S[1, 1]
        det = a * d - b * b
        lam_max = 0.5 * (a + d) + np.sqrt((0.5 * (a - d)) ** 2 + b * b)
        lam_min = 0.5 * (a + d) - np.sqrt((0.5 * (a - d)) ** 2 + b * b)
        cond["condition"] = max(cond["condition"], lam_max / lam_min)
        out["means_px"][i] = project(p, K)
        out["Sigmas_px"][i] = S
        out["Sigmas_inv"][i] = np.array([[d, -b], [-b, a]]) / det
        out["depths"][i] = z
        out["radii"][i] = cfg["radius_sigma"] * np.sqrt(lam_max)
        s = vmf_shading(centre - mu[i], np.asarray(batch["eta"], np.float64)[i]) if cfg["shade"] else 1.0
        out["colors"][i] = np.asarray(batch["color"], np.float64)[i] * s
        out["valid"][i] = 1
    return out, cond


def tile_lists(s, H, W, ts, cap):
    """Per tile: the survivors of the four strict bbox comparisons in the order (depth, index), cut at
    cap. Returns counts (T), survivors (T), indices (T, cap; -1 padded) and `cond`: the smallest bbox
    margin over every (valid splat, tile), the smallest relative difference of consecutive depths of a
    tile's survivors up to one past the cap (exact ties excluded; the tied index pairs, in list order, are
    collected), the most survivors."""
    tiles_x, T = W // ts, (H // ts) * (W // ts)
    counts, surv, idx = np.zeros(T, np.int32), np.zeros(T, np.int32), np.full((T, cap), -1, np.int32)
    cond = dict(bbox_margin=np.inf, depth_gap=np.inf, tie_pairs=set(), max_survivors=0, cut=0)
    ok = np.nonzero(s["valid"])[0]
    mx, my, r, z = s["means_px"][ok, 0], s["means_px"][ok, 1], s["radii"][ok], s["depths"][ok]
    for t in range(T):
        x0, y0 = float((t % tiles_x) * ts), float((t // tiles_x) * ts)
        sides = np.stack([(mx + r) - x0, (x0 + ts) - (mx - r), (my + r) - y0, (y0 + ts) - (my - r)])  # > 0: kept
        if ok.size:
            cond["bbox_margin"] = min(cond["bbox_margin"], float(np.abs(sides).min()))
        keep = (sides > 0).all(axis=0)
        order = ok[keep][np.lexsort((ok[keep], z[keep]))]
        surv[t], counts[t] = order.size, min(order.size, cap)
        idx[t, :counts[t]] = order[:cap]
        zs = s["depths"][order][:cap + 1]
        rel = np.diff(zs) / zs[1:]
        for j in np.nonzero(rel == 0)[0]:
            cond["tie_pairs"].add((int(order[j]), int(order[j + 1])))
        if (rel > 0).any():
            cond["depth_gap"] = min(cond["depth_gap"], float(rel[rel > 0].min()))
        cond["max_survivors"] = max(cond["max_survivors"], int(order.size))
        cond["cut"] += int(order.size > cap)
    return counts, surv, idx, cond


def composite_pixel(px, py, lst, s, cfg, cond=None):
    """One pixel centre over one list, in list order: (C (3), T, D, n)."""
    T, C, D, n = 1.0, np.zeros(3), 0.0, 0
    for i in lst:
        d = np.array([px, py]) - s["means_px"][i]
        Si = s["Sigmas_inv"][i]
        q = (d[0] * Si[0, 0] + d[1] * Si[1, 0]) * d[0] + (d[0] * Si[0, 1] + d[1] * Si[1, 1]) * d[1]
        a = min(cfg["alpha_max"], s["alphas"][i] * np.exp(-0.5 * max(q, 0.0)))
        if cond is not None:
            cond["skip_margin"] = min(cond["skip_margin"], abs(a - cfg["alpha_skip"]) / cfg["alpha_skip"])
        if a < cfg["alpha_skip"]:
            continue
        w = T * a
        C = C + w * s["colors"][i]
        D = D + w * s["depths"][i]
        n += 1
        T = T * (1.0 - a)
        if cond is not None:
            cond["stop_margin"] = min(cond["stop_margin"], abs(T - cfg["t_stop"]) / cfg["t_stop"])
        if T < cfg["t_stop"]:
            if cond is not None:
                cond["stopped"] += 1
            break
    return C, T, D, n


def raster(s, idx, counts, H, W, ts, cfg):
    """Every pixel of every tile over the tile's list. Returns images (H, W, 3), alpha, depth (H, W),
    n_contrib (H, W) int32 and `cond`: the smallest relative distance of an evaluated a from alpha_skip
    and of an updated T from t_stop, the number of pixels that stopped."""
    img, alpha, depth = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W))
    nc = np.zeros((H, W), np.int32)
    bg = np.asarray(cfg["background"], np.float64)
    cond = dict(skip_margin=np.inf, stop_margin=np.inf, stopped=0)
    tiles_x = W // ts
    for row in range(H):
        for col in range(W):
            t = (row // ts) * tiles_x + col // ts
            C, T, D, n = composite_pixel(col + 0.5, row + 0.5, idx[t, :counts[t]], s, cfg, cond)
            img[row, col] = C + T * bg
            alpha[row, col] = 1.0 - T
            depth[row, col] = D / (1.0 - T) if (1.0 - T) > cfg["eps"] else 0.0
            nc[row, col] = n
    return img, alpha, depth, nc, cond


def render(batch, Ks, T_cws, H, W, cfg):
    """Every view: the stacked prep arrays, lists and images (the device's shapes), and per view the
    conditions of prep, lists and raster merged into one dict."""
    ts, cap = cfg["tile_size"], cfg["max_splats_per_tile"]
    per, conds = [], []
    for K, T_cw in zip(Ks, T_cws):
        s, c0 = prep(batch, K, np.asarray(T_cw, np.float64), H, W, cfg)
        counts, surv, idx, c1 = tile_lists(s, H, W, ts, cap)
        img, alpha, depth, nc, c2 = raster(s, idx, counts, H, W, ts, cfg)
        per.append(dict(s, tile_counts=counts, tile_survivors=surv, tile_indices=idx, images=img, alpha=alpha,
                        depth=depth, n_contrib=nc))
        conds.append(dict(c0, **c1, **c2))
    out = {k: np.stack([p[k] for p in per]) for k in per[0] if k != "alphas"}
    out["alphas"] = per[0]["alphas"]
    return out, conds
