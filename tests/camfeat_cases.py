"""TEST INFRASTRUCTURE — the cases of the camera-feature tests (test_camera_features.py,
test_gpu_camera_features.py). Everything is drawn from fixed seeds.

The image has the size and intrinsics of camsplat_cases (96 x 72, fx = fy = 75) and a depth with the
same regions: a fronto-parallel wall at 4 m (left), a slanted wall z = 3 / (1 - 0.8 dx) (middle), a
floor y = 1.2 (right, below the horizon; the 4 m wall above it) and a far wall at 30 m in the lowest
fifth, plus a curved bump on the left wall, multiplicative noise of 0.4 %, float32 storage, 6 % of the
pixels set to 0, NaN, +inf or -1, one dead 8 x 8 block, and a few hand-made windows:

  COUNT_SPOTS   three pixels whose 3 x 3 window holds exactly 1, 3 and 4 valid values (the variance of a
                median window exists from 4 up)
  SPARSE_R2     a 7 x 7 window that is dead but for its centre and four of the hex offsets of radius 2:
                a valid depth (median or hex of radius 2) with 5 < quad_fit_min_points values to fit
  SPARSE_R3     the same for the hex offsets of radius 3

Keypoints are uniform over [-2, W + 1] x [-2, H + 1], after the hand-placed ones (HAND)."""

from __future__ import annotations

import numpy as np

import camfeat_restatement as RS
from camsplat_cases import CX, CY, FX, FY

W, H = 96, 72
K = (FX, FY, CX, CY)
DEPTH_SEED = 41
RGB_SEED = 43
KP_SEED = 47
DEAD_BLOCK = (40, 8)            # (x0, y0) of the dead 8 x 8 block, in the slanted wall
COUNT_SPOTS = {1: (8, 50), 3: (14, 50), 4: (20, 50)}
SPARSE_R2 = (27, 50)
SPARSE_R3 = (10, 40)

CASES = {
    "smallest": dict(cfg={}, m=1),
    "median3": dict(cfg={}, m=64),
    "median5": dict(cfg=dict(depth_sample_mode="median5"), m=64),
    "hex": dict(cfg=dict(depth_sample_mode="hex"), m=64),
    "nearest_quadratic": dict(cfg=dict(depth_sample_mode="nearest", depth_model="quadratic"), m=64),
    "unsaturated": dict(cfg=dict(kappa_alpha=0.05), m=64),
    "radius3": dict(cfg=dict(depth_sample_mode="hex", hex_radius=3, quad_fit_radius=3), m=64),
    "truncate": dict(cfg=dict(max_features=64), m=80),
}

# (u, v, response): halves in u and in v, the left edge, the corners, the hand-made windows, the dead
# block, responses <= 0
HAND = np.array([
    [30.5, 20.0, 180.0], [31.0, 21.5, 175.0], [-0.4, 30.0, 170.0], [-0.5, 30.0, 165.0],
    [0.0, 0.0, 160.0], [W - 1.0, 0.0, 158.0], [0.0, H - 1.0, 156.0], [W - 1.0, H - 1.0, 154.0],
    [COUNT_SPOTS[1][0] + 0.2, COUNT_SPOTS[1][1] - 0.3, 150.0], [COUNT_SPOTS[3][0] - 0.1, COUNT_SPOTS[3][1] + 0.4, 148.0],
    [COUNT_SPOTS[4][0] + 0.3, COUNT_SPOTS[4][1] + 0.1, 146.0],
    [SPARSE_R2[0] + 0.25, SPARSE_R2[1] - 0.25, 144.0], [SPARSE_R3[0] - 0.3, SPARSE_R3[1] + 0.2, 142.0],
    [DEAD_BLOCK[0] + 3.6, DEAD_BLOCK[1] + 4.1, 140.0], [22.3, 18.8, 138.0],
    [50.2, 40.7, 0.0], [70.6, 20.1, -3.0],
])


def _sparse(depth, centre, offsets):
    x, y = centre
    live = {(x + dx, y + dy): depth[y + dy, x + dx] for dx, dy in offsets}
    depth[y - 3:y + 4, x - 3:x + 4] = 0.0
    for (px, py), z in live.items():
        depth[py, px] = z if np.isfinite(z) and z > 0.0 else 4.0


def depth_image(seed=DEPTH_SEED):
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dx, dy = (u - CX) / FX, (v - CY) / FY
    z = np.full((H, W), 4.0)
    z -= 0.6 * np.exp(-((u - 22.0) ** 2 + (v - 19.0) ** 2) / (2.0 * 6.0 ** 2))      # the bump
    mid = (u >= 37.0) & (u < 66.0)
    z[mid] = 3.0 / (1.0 - 0.8 * dx[mid])
    floor = (u >= 66.0) & (v > 44.0)
    z[floor] = 1.2 / dy[floor]
    z[v >= 0.8 * H] = 30.0
    z *= 1.0 + 0.004 * rng.standard_normal((H, W))
    d = z.astype(np.float32)
    bad = rng.uniform(size=(H, W)) < 0.06
    d[bad] = rng.choice(np.array([0.0, np.nan, np.inf, -1.0], np.float32), size=int(bad.sum()))
    x0, y0 = DEAD_BLOCK
    d[y0:y0 + 8, x0:x0 + 8] = 0.0
    # exactly 1, 3 and 4 valid values in a 3 x 3 window
    for count, (x, y) in COUNT_SPOTS.items():
        live = [(0, 0), (1, 0), (-1, 1), (0, -1)][:count]
        d[y - 1:y + 2, x - 1:x + 2] = np.float32(np.nan)
        for ddx, ddy in live:
            d[y + ddy, x + ddx] = np.float32(4.0 + 0.01 * (ddx - 2 * ddy))
    _sparse(d, SPARSE_R2, RS.hex_offsets(2)[:5])
    _sparse(d, SPARSE_R3, RS.hex_offsets(3)[:5])
    return d


def rgb_image(seed=RGB_SEED):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def keypoints(m, seed=KP_SEED):
    if m == 1:
        return np.array([[30.5, 20.25, 80.0]])
    rng = np.random.default_rng(seed)
    n = m - HAND.shape[0]
    rand = np.stack([rng.uniform(-2.0, W + 1.0, n), rng.uniform(-2.0, H + 1.0, n), rng.uniform(5.0, 150.0, n)], axis=1)
    return np.concatenate([HAND, rand], axis=0)


def config(name):
    from gcslam.ops import VisualFeatureConfig
    return VisualFeatureConfig(**CASES[name]["cfg"])


_cache = {}


def build(name):
    """The case's inputs and the restatement's outputs for them (computed once per process, shared and
    not to be changed): depth, rgb, kp (all keypoints), kept (the rows select_keypoints keeps), cfg, ref."""
    if name not in _cache:
        from gcslam.ops import select_keypoints
        cfg = config(name)
        kp = keypoints(CASES[name]["m"])
        kept = select_keypoints(kp[:, 2], cfg.max_features)
        depth, rgb = depth_image(), rgb_image()
        _cache[name] = dict(name=name, depth=depth, rgb=rgb, kp=kp, kept=kept, cfg=cfg,
                            ref=RS.lift(depth, rgb, kp[kept], K, cfg))
    return _cache[name]


def err_frac(got, ref, bar, rows, scale_rows):
    """max |got - ref| over `rows` as a fraction of bar x max |ref| over `scale_rows` (the valid rows:
    the 1e6 of an invalid row's covariance would hide the rest)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = float(np.max(np.abs(ref[scale_rows]))) if scale_rows.any() else 0.0
    if not rows.any():
        return 0.0
    assert np.isfinite(ref[rows]).all() and np.isfinite(got[rows]).all()
    d = float(np.max(np.abs(got[rows] - ref[rows])))
    return d / (bar * scale) if scale > 0.0 else (0.0 if d == 0.0 else np.inf)
