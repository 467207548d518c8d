"""TEST INFRASTRUCTURE — the seeded inputs of the rendering tests, built on the CPU alone (the pattern
of camsplat_cases.py). tests/golden/make_render.py runs the reference on them and stores inputs and
outputs in tests/golden/render.npz; tests/test_render.py asserts the conditions under which they pin
an implementation; tests/test_gpu_render.py runs the device on them.

If a seeded case breaks a condition of tests/test_render.py, change its seed, not the margin."""

import os

import numpy as np

from oracle import gc_oracle as O

import render_restatement as RS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render.npz")
L = 3
EPS_LIFT = 1e-9

# ---------------------------------------------------------------------------------- tile drop-ins
# name -> (tile_size, tile origin (oy, ox), splat count, cap, seed)
TILE_CASES = {
    "t8_n0": (8, (8, 24), 0, 64, 1), "t8_n1": (8, (8, 24), 1, 64, 2), "t8_n5": (8, (8, 24), 5, 64, 3),
    "t8_n65": (8, (8, 24), 65, 64, 4), "t8_n257": (8, (8, 24), 257, 64, 5),
    "t32_n0": (32, (32, 64), 0, 64, 6), "t32_n257": (32, (32, 64), 257, 64, 8),
    "cap3": (8, (8, 24), 200, 3, 9), "cap64": (8, (8, 24), 200, 64, 10),
    "special": (8, (8, 24), 12, 64, 11),
}
# the cases whose render with splat_indices=None (every splat, in index order) is recorded too
NONE_LIST = ("t8_n0", "t8_n1", "t8_n5", "t8_n65", "t8_n257", "t32_n257")
FBM_TILE = dict(octaves=3, gain=0.6, seed=7, scale=0.3)  # the fBm colour modulation, recorded on FBM_TILE_CASE
FBM_TILE_CASE = "t8_n65"


def _sigma_inv(rng, n, lo, hi):
    """n symmetric 2 x 2 precisions with eigenvalues in [lo, hi] (condition number <= hi / lo)."""
    th = rng.uniform(0, np.pi, n)
    c, s = np.cos(th), np.sin(th)
    R = np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)
    ev = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 2)))
    S = np.einsum("nij,nj,nkj->nik", R, ev, R)
    return 0.5 * (S + np.swapaxes(S, 1, 2))


def build_tile(name):
    ts, (oy, ox), n, cap, seed = TILE_CASES[name]
    rng = np.random.default_rng(seed)
    overlap = name.startswith("cap")
    spread = 0.4 * ts if overlap else 1.2 * ts   # cap cases: every splat meets the tile (sigma >= 1 px)
    centre = np.array([ox + 0.5 * ts, oy + 0.5 * ts])
    means = centre + rng.uniform(-spread, spread, (n, 2))
    Sinv = _sigma_inv(rng, n, 0.02, 1.0) if n else np.zeros((0, 2, 2))   # sigma 1 .. 7 px
    alphas, colors = rng.uniform(0.05, 1.0, n), rng.uniform(0.0, 1.0, (n, 3))
    world = rng.uniform(-40.0, 40.0, (n, 2))
    if name == "special":
        means[0] = [ox - 50.0, oy - 50.0]                                  # wholly outside the tile
        Sinv[0] = np.diag([0.25, 0.25])
        means[3], means[7] = centre + [3.25, 1.5], centre + [-3.25, 1.5]   # mirrored: dist_sq exactly equal
        means[5] = centre + [2.0, -1.0]                                    # so tight that -q / 2 hits -log_clip
        Sinv[5] = np.diag([400.0, 300.0])
    return dict(tile_size=ts, origin=(oy, ox), cap=cap, means=means, Sigmas_inv=Sinv, alphas=alphas, colors=colors,
                world_xy=world)


# ----------------------------------------------------------------------------------------- fBm
FBM_RUNS = ((1, 0), (5, 0), (1, 7), (5, 7))  # (octaves, seed)
FBM_GAIN = 0.5
FBM_EXACT = 12  # the point whose x lies exactly on an integer


def build_fbm():
    rng = np.random.default_rng(21)
    xy = np.concatenate([rng.uniform(-3.0, 3.0, (16, 2)), rng.uniform(-40.0, 40.0, (8, 2)),
                         rng.uniform(990.0, 1010.0, (8, 2)), rng.uniform(-1010.0, -990.0, (8, 2)),
                         np.array([[-0.3, 0.6], [0.4, -0.7], [-1e-3, 1e-3]])])
    xy[FBM_EXACT] = [-7.0, 2.37]
    return xy


# ------------------------------------------------------------------------------------- BEV image
IMAGE = dict(H=64, W=96, tile_size=32, cap=16, n=300, origin_xy=(-2.0, -3.0), px_per_m=8.0, n_views=3,
             phi_center_deg=10.0, phi_span_deg=14.0, oblique_phi_deg=10.0, fbm_seed=7, fbm_modulate_scale=0.3)
PREP_ROWS = 40  # rows of the image batch on which the reference's pieces are recorded per view
RENDER_CFG = dict(tile_size=32, max_splats_per_tile=16, fbm_octaves=5, fbm_gain=0.5, opacity_gamma=1.0, logdet0=0.0,
                  eps=1e-12, ewa_log_clip=25.0, alpha_min=0.02)


def _sigma3(rng, n, lo, hi):
    Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    ev = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 3)))
    S = np.einsum("nij,nj,nkj->nik", Q, ev, Q)
    return 0.5 * (S + np.swapaxes(S, 1, 2))


def build_image_batch():
    """300 world-frame primitives over the viewport (12 m x 8 m at 8 px / m) and a little beyond."""
    rng = np.random.default_rng(31)
    n = IMAGE["n"]
    mu = np.column_stack([rng.uniform(-3.0, 11.0, n), rng.uniform(-4.0, 6.0, n), rng.uniform(-0.5, 2.0, n)])
    Sigma = _sigma3(rng, n, 0.01, 0.25)   # sigma 0.1 .. 0.5 m, condition number <= 25
    eta = rng.normal(size=(n, L, 3)) * 2.0
    eta[::7, 2] = 0.0                     # some lobes empty, as in a young map
    return dict(mu_world=mu, Sigma_world=Sigma, eta=eta, mass=rng.uniform(0.1, 1.0, n),
                color=rng.uniform(0.0, 1.0, (n, 3)), primitive_ids=np.arange(n, dtype=np.int64))


LOGDETS = np.linspace(-14.0, 8.0, 45)   # log det of a BEV covariance: sigma 1 mm .. 50 m
OPACITY_OTHER = dict(gamma=0.5, logdet0=-3.0, alpha_min=0.1)


def shading_inputs(batch, i):
    """(mu_app, kappa_app) of row i for vmf_shading_multi_lobe: eta_b and |eta_b| (a copy: the
    reference normalises mu_app in place)."""
    return batch["eta"][i].copy(), np.linalg.norm(batch["eta"][i], axis=1)


def image_views(single=False):
    """[(P, view_dir)] of the image case."""
    phis = [IMAGE["oblique_phi_deg"]] if single else RS.bev15_phis(IMAGE["n_views"], IMAGE["phi_center_deg"],
                                                                  IMAGE["phi_span_deg"])
    return [(RS.oblique_P(p), RS.view_dir(p)) for p in phis]


def restated_image(single=False):
    """The composition (render_restatement.bev_splats / render_image) over the image case's views."""
    b = build_image_batch()
    out = dict(images=[], counts=[], indices=[], splats=[], cond=[])
    for P, vd in image_views(single):
        s = RS.bev_splats(b, P, vd, IMAGE["origin_xy"], IMAGE["px_per_m"], RENDER_CFG, IMAGE["fbm_seed"],
                          IMAGE["fbm_modulate_scale"])
        img, cnt, idx, cond = RS.render_image(s, IMAGE["H"], IMAGE["W"], IMAGE["tile_size"], IMAGE["cap"],
                                              RENDER_CFG["ewa_log_clip"], RENDER_CFG["eps"])
        for k, v in zip(("images", "counts", "indices", "splats", "cond"), (img, cnt, idx, s, cond)):
            out[k].append(v)
    return out


# ------------------------------------------------------------------------------ renderable batch
M_TILE = 32


def build_map(empty=False):
    """{tile key: tile} of three tiles of m_tile = 32: one empty, one full, one half full; ids unique
    over the map, several slots sharing each last_supported_scan_seq, all weights distinct."""
    rng = np.random.default_rng(41)
    tiles = {}
    for j, (key, n_valid) in enumerate(((11, 0), (5, M_TILE), (8, M_TILE // 2))):
        t = O.empty_tile(M_TILE, L)
        if n_valid and not empty:
            slots = np.sort(rng.permutation(M_TILE)[:n_valid])
            B = rng.normal(size=(n_valid, 3, 3)) * 0.3
            Lam = B @ np.swapaxes(B, 1, 2) + 2.0 * np.eye(3)
            t["Lambdas"][slots] = Lam
            t["thetas"][slots] = np.einsum("nij,nj->ni", Lam, rng.uniform(-3.0, 3.0, (n_valid, 3)))
            t["etas"][slots] = rng.normal(size=(n_valid, L, 3)) * 2.0
            t["weights"][slots] = rng.permutation(n_valid) * 0.01 + 0.1 + 0.003 * j
            t["valid_mask"][slots] = True
            t["primitive_ids"][slots] = 1000 * j + rng.permutation(n_valid)
            t["last_supported_scan_seq"][slots] = rng.integers(0, 5, n_valid)
            t["rgb"][slots] = rng.uniform(0.0, 1.0, (n_valid, 3))
        tiles[key] = t
    return tiles


def expected_batch(tiles, tile_ids, m_tile_view):
    view = O.extract_atlas_map_view(tiles, tile_ids, m_tile_view, M_TILE, L, eps_lift=EPS_LIFT)
    return RS.publish(view, EPS_LIFT), view


# --------------------------------------------------------------------------------------- helpers
def err(got, want):
    """max |got - want|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want))) if want.size else 0.0


def err_rel(got, want):
    """max |got - want| / max |want|"""
    want = np.asarray(want, np.float64)
    return err(got, want) / max(float(np.max(np.abs(want))) if want.size else 0.0, 1e-300)
