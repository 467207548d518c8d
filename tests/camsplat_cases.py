"""TEST INFRASTRUCTURE — the cases of the camera-splat tests (test_camera_splats.py,
test_gpu_camera_splats.py) and of tests/golden/make_camera_splats.py, which records the reference's
outputs for exactly these inputs. Everything is drawn from fixed seeds; the fixture stores the
inputs too, and test_camera_splats.py checks that they are the ones built here.

The scene: a 96 x 72 image, fx = fy = 75, 1,536 LiDAR points whose pixels are uniform over the image
without the column strip u < 8. Depth by image region: a fronto-parallel wall at 4 m (left), a
slanted wall z = 3 / (1 - 0.8 dx) (middle), a floor y = 1.2 (right, below the horizon; the 4 m wall
above it) and a far wall at 30 m in the lowest fifth. Range noise 0.01 z / 4. The first 1/16 of the
points are mirrored behind the camera; one point has z exactly 0."""

from __future__ import annotations

import os

import numpy as np

from camsplat_restatement import to_camera_frame

W, H = 96.0, 72.0
FX = FY = 75.0
CX, CY = 48.0, 36.0
N_POINTS = 1536
SCENE_SEED = 4
QUERY_SEED = 11
FEATURE_SEED = 23
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_splats.npz")

# base <- camera: a camera looking along the base frame's x, 8 degrees of pitch, a lever arm
_c, _s = np.cos(np.deg2rad(8.0)), np.sin(np.deg2rad(8.0))
R_BASE_CAMERA = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]) @ np.array(
    [[1.0, 0.0, 0.0], [0.0, _c, -_s], [0.0, _s, _c]])
T_BASE_CAMERA = np.array([0.21, -0.04, 0.35])
TIMESTAMP = 1712.125
EPS_LIFT = 1e-9

CASES = {
    "smallest": dict(cfg={}, n_feat=4, n_surfel=2, n_query=1),
    "mixed": dict(cfg={}, n_feat=64, n_surfel=32, n_query=60),
    "select": dict(cfg=dict(lidar_ray_plane_fit_max_points=8, lidar_projection_radius_pix=4.0, gamma_lidar=0.7),
                   n_feat=64, n_surfel=32, n_query=60, weights=True),
    "truncate": dict(cfg={}, n_feat=64, n_surfel=32, n_query=70),
    "pad": dict(cfg={}, n_feat=64, n_surfel=32, n_query=20),
}


def scene(seed=SCENE_SEED, n=N_POINTS):
    rng = np.random.default_rng(seed)
    u = rng.uniform(8.0, W, n)
    v = rng.uniform(0.0, H, n)
    dx, dy = (u - CX) / FX, (v - CY) / FY
    z = np.full(n, 4.0)
    mid = (u >= 37.0) & (u < 66.0)
    z[mid] = 3.0 / (1.0 - 0.8 * dx[mid])
    floor = (u >= 66.0) & (v > 44.0)
    z[floor] = 1.2 / dy[floor]
    z[v >= 0.8 * H] = 30.0
    z = z + rng.standard_normal(n) * (0.01 * z / 4.0)
    p = np.stack([dx * z, dy * z, z], axis=1)
    p[: n // 16] *= -1.0           # behind the camera
    p[n // 16, 2] = 0.0            # z exactly 0
    return p


def queries(n, seed=QUERY_SEED):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.0, W, n), rng.uniform(0.0, H, n)], axis=1)


def features(uv, seed=FEATURE_SEED):
    """The CameraFeatures arrays for the pixels uv: every second feature has Λ_c = 0, every third no
    mu_app, every fourth no colour; colours from [-0.1, 1.1]."""
    rng = np.random.default_rng(seed)
    m = uv.shape[0]
    i = np.arange(m)
    z_c = rng.uniform(2.0, 8.0, m)
    Lc = np.where(i % 2 == 1, 0.0, 1.0 / (0.05 * z_c) ** 2)
    mu = rng.standard_normal((m, 3))
    mu /= np.linalg.norm(mu, axis=1)[:, None]
    has_mu = i % 3 != 2
    mu[~has_mu] = 0.0
    has_color = i % 4 != 3
    color = rng.uniform(-0.1, 1.1, (m, 3))
    color[~has_color] = 0.0
    A = rng.standard_normal((m, 3, 3)) * 0.05
    return dict(u=uv[:, 0].copy(), v=uv[:, 1].copy(), depth_Lambda_c=Lc, depth_theta_c=Lc * z_c,
                weight=rng.uniform(0.2, 1.0, m), kappa_app=rng.uniform(0.5, 20.0, m), mu_app=mu, has_mu_app=has_mu,
                color=color, has_color=has_color, xyz=rng.uniform(0.5, 5.0, (m, 3)),
                cov_xyz=A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)[None])


def build(name):
    c = CASES[name]
    if name == "smallest":
        pts = np.array([[0.10, -0.05, 2.0], [0.12, -0.02, 2.05], [0.07, -0.03, 1.98]])
        uv = np.array([[CX + FX * 0.05, CY - FY * 0.015]])
    else:
        pts = scene()
        uv = queries(c["n_query"])
    # the operator's input is the base-frame cloud; the camera-frame points are the node's own
    # expression of it (backend_node.py:1876), so they differ from pts in the last bits
    base = pts @ R_BASE_CAMERA.T + T_BASE_CAMERA
    out = dict(name=name, points_cam=to_camera_frame(base, R_BASE_CAMERA, T_BASE_CAMERA), points_base=base, uv=uv,
               cfg=dict(c["cfg"]), n_feat=c["n_feat"], n_surfel=c["n_surfel"], features=features(uv),
               point_weights=None)
    if c.get("weights"):
        out["point_weights"] = np.random.default_rng(31).uniform(0.2, 2.0, pts.shape[0])
    return out


INPUT_KEYS = ("points_cam", "points_base", "uv", "point_weights")


def load(name, golden=None):
    """The case as the fixture stores it: its inputs and the reference's recorded outputs
    (ref_* keys), with points_cam the node's camera-frame points of points_base."""
    g = golden if golden is not None else np.load(GOLDEN)
    c = build(name)
    pre = name + "/"
    out = dict(name=name, cfg=c["cfg"], n_feat=c["n_feat"], n_surfel=c["n_surfel"], point_weights=None)
    for k in g.files:
        if k.startswith(pre):
            out[k[len(pre):]] = g[k]
    for k in ("points_base", "points_cam"):
        if k not in out:  # stored once for the cases that share the scene
            out[k] = g["scene/" + k]
    out["features"] = {k[5:]: out.pop(k) for k in list(out) if k.startswith("feat_")}
    return out


def config(case):
    from gcslam.ops import LidarCameraDepthFusionConfig
    return LidarCameraDepthFusionConfig(**case["cfg"])


def restated(case, weighted=True):
    """The restatement's evidence (with its `cond` record) for a case's camera-frame points."""
    import camsplat_restatement as RS
    pw = case.get("point_weights") if weighted else None
    return RS.evidence(case["points_cam"], case["uv"], FX, FY, CX, CY, config(case), pw)


def expected_batch(case, xyz_cam=None, cov_cam=None):
    """The batch of the case: the recorded splat_prep_fused outputs through the restated base-frame
    loop and batch builder."""
    import camsplat_restatement as RS
    return RS.camera_batch(case["features"], case["ref_fused_xyz"] if xyz_cam is None else xyz_cam,
                           case["ref_fused_cov"] if cov_cam is None else cov_cam, R_BASE_CAMERA, T_BASE_CAMERA,
                           TIMESTAMP, case["n_feat"], case["n_surfel"], EPS_LIFT)


def err_frac(got, ref, bar, rows=None):
    """max |got - ref| as a fraction of bar x max |ref| (over the finite entries of the whole
    reference array); the non-finite entries must sit in the same places with the same values."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = np.isfinite(ref)
    scale = float(np.max(np.abs(ref[fin]))) if fin.any() else 0.0
    if rows is not None:
        got, ref, fin = got[rows], ref[rows], fin[rows]
    assert np.array_equal(np.isfinite(got), fin)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    if not fin.any():
        return 0.0
    d = float(np.max(np.abs(got[fin] - ref[fin])))
    return d / (bar * scale) if scale > 0.0 else (0.0 if d == 0.0 else np.inf)
