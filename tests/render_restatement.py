"""TEST INFRASTRUCTURE — a NumPy restatement of the reference's output side, vectorised, with the
lines it restates:

  backend/rendering.py          opacity_from_logdet :236-244, vmf_shading_multi_lobe :117-159,
                                _hash_float / _value_noise_2d / fbm_value_noise :167-209,
                                splat_indices_for_tile :252-289, render_tile_ewa :297-355
  common/bev_pushforward.py     pushforward_gaussian_3d_to_2d :42-64, _oblique_P :30-39
  backend/map_publisher.py      publish :143-242 (the ordering :200 and the batch :224-242)

and the composition the reference leaves open and this build defines (bev_splats and
render_image below). tests/test_render.py holds every restated piece to the reference's recorded
outputs (tests/golden/render.npz) at 1e-12; the GPU tests compare the device with the recorded
outputs where the reference pins them and with this file where only the composition does."""

import numpy as np


# ------------------------------------------------------------------------------ rendering.py
def opacity_from_logdet(logdet_cov, gamma=1.0, logdet0=0.0, alpha_min=0.02):
    """:243-244"""
    raw = 1.0 / (1.0 + np.exp(-gamma * (logdet0 - np.asarray(logdet_cov, np.float64))))
    return alpha_min + (1.0 - alpha_min) * raw


def vmf_shading(v, eta, eps=1e-12):
    """:135-159 with pi_b=None and no intensity, mu_app = eta_b, kappa_app = |eta_b|. v (3,), eta (N, B, 3)."""
    v = np.asarray(v, np.float64) / (np.linalg.norm(v) + eps)
    kap = np.linalg.norm(eta, axis=-1)                     # (N, B)
    mu = eta / (kap[..., None] + eps)
    B = eta.shape[1]
    s = np.sum(np.exp(kap * (mu @ v - 1.0)) / B, axis=1)
    return s / (1.0 + kap.sum(axis=1) / max(B, 1))


def _hash_float(h):
    """:167-170 on int64 (h < 2^31: the product stays below 2^62)."""
    h = (h * 1103515245 + 12345) & 0x7FFFFFFF
    return h.astype(np.float64) / float(0x7FFFFFFF + 1)


def _value_noise_2d(x, y, seed):
    """:173-188. int64 two's complement & 0x7FFFFFFF equals Python's mask of the unbounded integer."""
    fl_x, fl_y = np.floor(x), np.floor(y)
    ix, iy = fl_x.astype(np.int64), fl_y.astype(np.int64)
    fx, fy = np.clip(x - fl_x, 0.0, 1.0), np.clip(y - fl_y, 0.0, 1.0)
    cell = lambda a, b: _hash_float(((seed * 31 + a) * 31 + b) & 0x7FFFFFFF)
    v00, v10, v01, v11 = cell(ix, iy), cell(ix + 1, iy), cell(ix, iy + 1), cell(ix + 1, iy + 1)
    sx, sy = fx * fx * (3.0 - 2.0 * fx), fy * fy * (3.0 - 2.0 * fy)
    v0 = v00 * (1 - sx) + v10 * sx
    v1 = v01 * (1 - sx) + v11 * sx
    return v0 * (1 - sy) + v1 * sy


def fbm(xy, octaves=5, gain=0.5, seed=0):
    """:191-228"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    value, amplitude, frequency, max_amplitude = np.zeros(xy.shape[0]), 1.0, 1.0, 0.0
    for _ in range(int(octaves)):
        value = value + amplitude * _value_noise_2d(xy[:, 0] * frequency, xy[:, 1] * frequency, int(seed))
        max_amplitude += amplitude
        amplitude *= gain
        frequency *= 2.0
    return value / (max_amplitude + 1e-12)


def fbm_integer_margin(xy, octaves):
    """The smallest distance of any scaled coordinate from an integer, over the octaves."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    m = np.full(xy.shape, np.inf)
    for o in range(int(octaves)):
        s = xy * 2.0 ** o
        m = np.minimum(m, np.abs(s - np.round(s)))
    return m


def tile_bins(tile_origin, tile_size, means, Sigmas_inv, cap=64, eps=1e-12):
    """:266-289, and what the conditions of tests/test_render.py read: the smallest margin of the four
    bbox comparisons, and the smallest relative gap between consecutive dist_sq of the survivors up to
    one past the cap (exact ties excluded and counted)."""
    oy, ox = int(tile_origin[0]), int(tile_origin[1])
    ts = min(max(int(tile_size), 1), 32)
    means = np.asarray(means, np.float64).reshape(-1, 2)
    N = means.shape[0]
    if N == 0:
        return np.zeros(0, np.int64), dict(margin=np.inf, gap=np.inf, ties=0, survivors=0)
    lam = np.maximum(np.linalg.eigvalsh(np.asarray(Sigmas_inv, np.float64).reshape(N, 2, 2))[:, 0], eps)
    r = 2.0 / np.sqrt(lam)
    mx, my = means[:, 0], means[:, 1]
    sides = np.stack([ox - (mx + r), (mx - r) - (ox + ts), oy - (my + r), (my - r) - (oy + ts)])  # > 0: rejected
    keep = ~(sides > 0).any(axis=0)
    d = (mx - (ox + 0.5 * ts)) ** 2 + (my - (oy + 0.5 * ts)) ** 2
    idx = np.nonzero(keep)[0]
    order = idx[np.argsort(d[idx], kind="stable")]
    ds = d[order][:cap + 1]
    rel = np.diff(ds) / np.maximum(ds[1:], 1e-300)
    ties = int((rel == 0).sum())
    gap = float(rel[rel > 0].min()) if (rel > 0).any() else np.inf
    return order[:cap].astype(np.int64), dict(margin=float(np.abs(sides).min()), gap=gap, ties=ties,
                                              survivors=int(keep.sum()))


def render_tile(tile_origin, tile_size, means, Sigmas_inv, alphas, colors, splat_indices=None, log_clip=25.0):
    """:320-355 (the colours already modulated)."""
    ts = min(max(int(tile_size), 1), 32)
    out = np.zeros((ts, ts, 3))
    N = np.shape(means)[0]
    if N == 0 or (splat_indices is not None and len(splat_indices) == 0):
        return out
    idx = np.arange(N) if splat_indices is None else np.asarray(splat_indices, np.int64)
    m, S = np.asarray(means, np.float64).reshape(N, 2)[idx], np.asarray(Sigmas_inv, np.float64).reshape(N, 2, 2)[idx]
    a, c = np.asarray(alphas, np.float64)[idx], np.asarray(colors, np.float64).reshape(-1, 3)[idx]
    oy, ox = tile_origin
    py, px = np.meshgrid(np.arange(ts), np.arange(ts), indexing="ij")
    p = np.stack([ox + px + 0.5, oy + py + 0.5], axis=-1)           # (ts, ts, 2)
    d = p[:, :, None, :] - m[None, None]                            # (ts, ts, n, 2)
    q = np.einsum("yxni,nij,yxnj->yxn", d, S, d)
    w = a * np.exp(np.clip(-0.5 * np.maximum(q, 0.0), -log_clip, 0.0))
    total = w.sum(axis=-1) + 1e-12
    out = np.einsum("yxn,nc->yxc", w, c)
    out = np.where((total > 1e-12)[..., None], out / total[..., None], out)
    return np.clip(out, 0.0, 1.0)


# ------------------------------------------------------------------------ bev_pushforward.py
def oblique_P(phi_deg):
    """:30-39"""
    phi = np.deg2rad(float(phi_deg))
    return np.array([[1.0, 0.0, 0.0], [0.0, np.cos(phi), np.sin(phi)]])


def bev15_phis(n_views=15, center=10.0, span=14.0):
    """:78-86"""
    n = max(1, int(n_views))
    return np.array([center]) if n == 1 else center + np.linspace(-0.5, 0.5, n) * span


def pushforward(mu, Sigma, P):
    """:62-63, batched over the Gaussians."""
    return mu @ P.T, P @ Sigma @ P.T


# ----------------------------------------------------------------------------- map_publisher.py
def publish(view, eps_lift):
    """:194-242 from the arrays of an AtlasMapView (oracle.extract_atlas_map_view): the valid entries
    in the order np.lexsort((primitive_ids, -last_supported_scan_seq))."""
    ok = np.nonzero(np.asarray(view["valid_mask"], bool))[0]
    ids, seq = view["primitive_ids"][ok], view["last_supported_scan_seq"][ok]
    sel = ok[np.lexsort((ids, -seq))]
    Sigma = view["covariances"][sel]
    Lam = np.linalg.inv(Sigma + eps_lift * np.eye(3)[None]) if sel.size else np.zeros((0, 3, 3))
    return dict(mu_world=view["positions"][sel], Sigma_world=Sigma, Lambda_world=Lam, eta=view["etas"][sel],
                mass=view["weights"][sel], color=view["colors"][sel], primitive_ids=view["primitive_ids"][sel],
                last_supported_scan_seq=view["last_supported_scan_seq"][sel])


# ------------------------------------------------------------- the build-defined composition
def bev_splats(batch, P, view_dir, origin_xy, px_per_m, cfg, fbm_seed=0, fbm_modulate_scale=0.0):
    """One view's 2D splats: means_px = (P mu - origin) px_per_m, Sigmas_inv = the
    closed-form inverse of px_per_m^2 Sigma_bev + eps I, alphas from log det Sigma_bev, colors =
    color * shading(view_dir) * ((1 - s_f) + s_f fbm(world x, y)). cfg: the SplatRenderingConfig fields."""
    mu_bev, S_bev = pushforward(batch["mu_world"], batch["Sigma_world"], P)
    means = (mu_bev - np.asarray(origin_xy, np.float64)) * px_per_m
    A = px_per_m ** 2 * S_bev + cfg["eps"] * np.eye(2)
    det = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    Sinv = np.stack([A[:, 1, 1], -A[:, 0, 1], -A[:, 1, 0], A[:, 0, 0]], axis=-1).reshape(-1, 2, 2) / det[:, None, None]
    logdet = np.log(S_bev[:, 0, 0] * S_bev[:, 1, 1] - S_bev[:, 0, 1] * S_bev[:, 1, 0])
    alphas = opacity_from_logdet(logdet, cfg["opacity_gamma"], cfg["logdet0"], cfg["alpha_min"])
    f = fbm(batch["mu_world"][:, :2], cfg["fbm_octaves"], cfg["fbm_gain"], fbm_seed)
    mod = (1.0 - fbm_modulate_scale) + fbm_modulate_scale * f
    colors = batch["color"] * vmf_shading(view_dir, batch["eta"])[:, None] * mod[:, None]
    return dict(means_px=means, Sigmas_inv=Sinv, alphas=alphas, colors=colors, fbm=f, Sigmas_bev=S_bev)


def view_dir(phi_deg):
    """The null vector of P(phi)."""
    phi = np.deg2rad(float(phi_deg))
    return np.array([0.0, -np.sin(phi), np.cos(phi)])


def render_image(splats, H, W, tile_size, cap, log_clip, eps):
    """One view: every tile's list (tile_bins) and raster (render_tile). Returns the image, the counts
    (T), the indices (T, cap; -1 padded) and the worst conditions over the tiles."""
    ts = int(tile_size)
    img = np.zeros((H, W, 3))
    T = (H // ts) * (W // ts)
    counts, indices = np.zeros(T, np.int32), np.full((T, cap), -1, np.int32)
    cond = dict(margin=np.inf, gap=np.inf, ties=0, cut=0)
    for t in range(T):
        oy, ox = (t // (W // ts)) * ts, (t % (W // ts)) * ts
        idx, c = tile_bins((oy, ox), ts, splats["means_px"], splats["Sigmas_inv"], cap, eps)
        counts[t], indices[t, :len(idx)] = len(idx), idx
        cond["margin"], cond["gap"] = min(cond["margin"], c["margin"]), min(cond["gap"], c["gap"])
        cond["ties"] += c["ties"]
        cond["cut"] += int(c["survivors"] > cap)
        img[oy:oy + ts, ox:ox + ts] = render_tile((oy, ox), ts, splats["means_px"], splats["Sigmas_inv"],
                                                  splats["alphas"], splats["colors"], idx, log_clip)
    return img, counts, indices, cond
