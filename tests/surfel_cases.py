"""Seeded inputs of the surfel-extraction tests (test_surfels.py, test_gpu_surfels.py) and the
preconditions they assert on the restatement alone before any comparison.

The synthetic scene: a floor at z = -0.37 over [-1, 1]^2, a wall at x = 0.93 (y in [-1, 1], z in
[-0.5, 0.5]) and a slanted plane z = 0.3 x + 0.2 y + 0.41 over [-1, 1]^2 in equal thirds, 3 mm
isotropic noise, shuffled; w ~ U(0.2, 1), t ~ U(0, 0.1); every 97th point set to 1e6 (the parser's
non-finite sentinel), so the mask is exercised.

Preconditions (check_conditions):
 1. every unmasked point's s/h lies >= 1e-9 from an integer on all three axes: the centre's
    summation order differs by ulps between the two sides, cell membership must not;
 2. a valid cell is orientation-determined when (λ1 - λ0)/λ2 >= 1e-4, |n_z| >= 1e-6 and
    ||n_z| - 0.9| >= 1e-6 (the sign flip and the basis switch are then the same on both sides, and a
    1e-4 gap amplifies an ulp-level perturbation of the covariance to about 1e-12); the
    normal-dependent fields are compared only on such cells;
 3. at most 2 % of a case's valid cells may fail 2."""

import functools

import numpy as np

import surfel_restatement as SR

MARGIN_MIN = 1e-9
UNDETERMINED_MAX_FRAC = 0.02


def scene(n, seed=0):
    rng = np.random.default_rng(seed)
    k = n // 3
    sizes = (k, k, n - 2 * k)
    xy = [rng.uniform(-1.0, 1.0, (m, 2)) for m in sizes]
    floor = np.column_stack([xy[0], np.full(sizes[0], -0.37)])
    wall = np.column_stack([np.full(sizes[1], 0.93), xy[1][:, 0], 0.5 * xy[1][:, 1]])
    slant = np.column_stack([xy[2], 0.3 * xy[2][:, 0] + 0.2 * xy[2][:, 1] + 0.41])
    pts = np.concatenate([floor, wall, slant]) + rng.normal(scale=0.003, size=(n, 3))
    pts = pts[rng.permutation(n)]
    w = rng.uniform(0.2, 1.0, n)
    t = rng.uniform(0.0, 0.1, n)
    pts[::97] = SR.SENTINEL
    return pts, t, w


_SMALL = dict(n_surfel=64, n_feat=4, voxel_size_m=0.25, hex3d_num_cells_1=8, hex3d_num_cells_2=8,
              hex3d_num_cells_z=4, hex3d_max_occupants=8)
NAMES = ("smoke", "overflow_truncate", "default_grid", "kappa_open", "empty_sentinel", "empty_weightless")


@functools.lru_cache(maxsize=None)
def build(name):
    """dict(points, timestamps, weights, cfg): cfg holds SurfelExtractionConfig fields."""
    if name == "smoke":  # test_lidar_surfel_extraction_mahex3d.py:18-34
        rng = np.random.default_rng(0)
        a = rng.normal(loc=[0.0, 0.0, 0.0], scale=0.01, size=(20, 3))
        b = rng.normal(loc=[1.0, 1.0, 0.0], scale=0.01, size=(20, 3))
        pts = np.vstack([a, b]).astype(np.float64)
        return dict(points=pts, timestamps=np.linspace(0.0, 1.0, 40), weights=np.ones(40),
                    cfg=dict(n_surfel=8, n_feat=4, voxel_size_m=0.5, min_points_per_voxel=5, hex3d_num_cells_1=8,
                             hex3d_num_cells_2=8, hex3d_num_cells_z=2, hex3d_max_occupants=32))
    if name in ("overflow_truncate", "kappa_open"):
        p, t, w = scene(4096, 0)
        cfg = dict(_SMALL, kappa_main_scale=0.05) if name == "kappa_open" else dict(_SMALL)
        return dict(points=p, timestamps=t, weights=w, cfg=cfg)
    if name == "default_grid":
        p, t, w = scene(8192, 0)
        return dict(points=p, timestamps=t, weights=w, cfg={})
    if name == "empty_sentinel":
        p, t, w = scene(64, 0)
        return dict(points=np.full((64, 3), SR.SENTINEL), timestamps=t, weights=w, cfg=dict(_SMALL))
    if name == "empty_weightless":
        p, t, w = scene(64, 0)
        return dict(points=p, timestamps=t, weights=np.zeros(64), cfg=dict(_SMALL))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement of a case, computed once and shared; treat it as read-only."""
    c = build(name)
    return SR.extract(c["points"], c["timestamps"], c["weights"], c["cfg"])


def stats(ref):
    v = ref["cell_valid"]
    return dict(n_cells=int(v.shape[0]), valid=int(v.sum()), overflow=int((ref["count"] > ref["count_used"]).sum()),
                undetermined=int((v & ~ref["cell_determined"]).sum()),
                margin=float(ref["point_margin"][ref["mask"]].min()) if ref["mask"].any() else float("inf"))


def check_conditions(ref):
    s = stats(ref)
    assert s["margin"] >= MARGIN_MIN, s
    assert s["undetermined"] <= UNDETERMINED_MAX_FRAC * max(s["valid"], 1), s
    return s
