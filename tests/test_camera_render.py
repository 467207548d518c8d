"""The camera view without a GPU: the restatement (tests/camrender_restatement.py) against closed forms,
the conditions under which the seeded cases (tests/camrender_cases.py) pin an implementation, each case
reaching its branch, and every argument error of gcslam.rendering's camera entries raised with no
device. tests/test_gpu_camera_render.py holds the device to the restatement on the same cases.

The conditions bound how close an input may come to a discontinuity of the definitions (a bbox
comparison, the depth order, alpha_skip, t_stop, near and far): an implementation whose rounding differs
in the last bits then takes the same branches, and the 1e-10 parity bar of the GPU tests is meaningful.
They are asserted on the restatement alone."""

import dataclasses
import types

import numpy as np
import pytest

import camrender_cases as CC
import camrender_restatement as CS
from gcslam import _abi
from gcslam import rendering as R
from gcslam.ops.camera_splats import PinholeIntrinsics


def _one(mu, Sigma, color, mass=1.0):
    n = len(mu)
    return dict(mu_world=np.asarray(mu, np.float64), Sigma_world=np.asarray(Sigma, np.float64),
                eta=np.zeros((n, 1, 3)), mass=np.full(n, mass) if np.isscalar(mass) else np.asarray(mass, np.float64),
                color=np.asarray(color, np.float64))


# ------------------------------------------------------------------------------- closed forms
def test_isotropic_splat_on_the_axis():
    """Sigma = s^2 I at (0, 0, z0), R = I: Sigma_px = ((fx s / z0)^2 + lowpass) I at (cx, cy), so
    alpha(pixel) = exp(-d^2 / (2 ((fx s / z0)^2 + lowpass))), cut at alpha_skip; image = alpha color;
    depth = z0. The depth is D / (1 - T) with T = 1 - a rounded, so 1 - T is a to within 2^-53 absolute and
    the quotient is z0 to within 2^-53 / alpha_skip + 2 roundings relative (< 4e-14), not to the bit."""
    s, z0, K = 0.2, 4.0, (60.0, 60.0, 32.0, 32.0)
    color = np.array([[0.9, 0.5, 0.1]])
    cfg = CS.config(alpha_max=1.0, shade=False)
    out, _ = CS.render(_one([[0.0, 0.0, z0]], [np.eye(3) * s * s], color), [K], [np.eye(4)], 48, 64, cfg)
    var = (K[0] * s / z0) ** 2 + cfg["lowpass_px2"]
    rows, cols = np.meshgrid(np.arange(48) + 0.5, np.arange(64) + 0.5, indexing="ij")
    want = np.exp(-0.5 * ((cols - K[2]) ** 2 + (rows - K[3]) ** 2) / var)
    want[want < cfg["alpha_skip"]] = 0.0
    assert np.abs(np.abs(want - cfg["alpha_skip"]) / cfg["alpha_skip"])[want > 0].min() > 1e-9
    # exp(-9 / 2) > alpha_skip: the 3-sigma box cuts by tile, not by pixel. Here the mean lies on a tile
    # corner and the box meets the four tiles around it, which hold every pixel with alpha >= alpha_skip
    assert K[2] % 16 == 0 and K[3] % 16 == 0 and np.sqrt(-2.0 * np.log(cfg["alpha_skip"]) * var) < 16.0
    assert out["tile_survivors"][0].sum() == 4
    assert (want > 0).sum() > 100 and (want == 0).sum() > 100
    np.testing.assert_allclose(out["alpha"][0], want, rtol=0, atol=1e-14)
    np.testing.assert_allclose(out["images"][0], want[..., None] * color[0], rtol=0, atol=1e-14)
    hit = want > 0
    assert np.max(np.abs(out["depth"][0][hit] / z0 - 1.0)) < 4e-14 and not out["depth"][0][~hit].any()
    np.testing.assert_array_equal(out["n_contrib"][0], hit.astype(np.int32))
    np.testing.assert_allclose(out["Sigmas_px"][0, 0], var * np.eye(2), rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(out["radii"][0, 0], 3.0 * np.sqrt(var), rtol=1e-14)


K_TWO = (60.0, 60.0, 8.0, 8.0)


def _two(z_a, z_b, swap_index=False):
    """Two broad splats over the centre pixel: A (red, mass 1) at z_a, B (blue, mass 0.5) at z_b."""
    mu = [[0.02, 0.01, z_a], [-0.03, 0.02, z_b]]
    Sig = [np.eye(3) * 0.09, np.eye(3) * 0.16]
    col, mass = [[1.0, 0.1, 0.0], [0.0, 0.2, 1.0]], [1.0, 0.5]
    if swap_index:
        mu, Sig, col, mass = mu[::-1], Sig[::-1], col[::-1], mass[::-1]
    cfg = CS.config(shade=False)
    out, _ = CS.render(_one(mu, Sig, col, mass), [K_TWO], [np.eye(4)], 16, 16, dict(cfg))
    return out


def test_two_splats_over_one_pixel():
    """a1 c1 + (1 - a1) a2 c2 in depth order; exchanging the indices changes nothing, exchanging the depths
    does."""
    K = K_TWO
    out = _two(3.0, 5.0)
    r, c = 7, 9
    px = np.array([c + 0.5, r + 0.5])

    def a_of(mu, var3, alpha):
        m = np.array([K[0] * mu[0] / mu[2] + K[2], K[1] * mu[1] / mu[2] + K[3]])
        J = np.array([[K[0] / mu[2], 0, -K[0] * mu[0] / mu[2] ** 2], [0, K[1] / mu[2], -K[1] * mu[1] / mu[2] ** 2]])
        S = var3 * J @ J.T + 0.3 * np.eye(2)
        d = px - m
        return min(0.99, alpha * np.exp(-0.5 * d @ np.linalg.solve(S, d)))

    def blend(zA, zB):
        aA, aB = a_of([0.02, 0.01, zA], 0.09, 1.0), a_of([-0.03, 0.02, zB], 0.16, 0.5)
        cA, cB = np.array([1.0, 0.1, 0.0]), np.array([0.0, 0.2, 1.0])
        first = (aA, cA, zA, aB, cB, zB) if zA < zB else (aB, cB, zB, aA, cA, zA)
        a1, c1, z1, a2, c2, z2 = first
        cov = a1 + (1 - a1) * a2
        return a1 * c1 + (1 - a1) * a2 * c2, cov, (a1 * z1 + (1 - a1) * a2 * z2) / cov

    img, cov, dep = blend(3.0, 5.0)
    np.testing.assert_allclose(out["images"][0, r, c], img, rtol=1e-12)
    np.testing.assert_allclose(out["alpha"][0, r, c], cov, rtol=1e-12)
    np.testing.assert_allclose(out["depth"][0, r, c], dep, rtol=1e-12)
    assert out["n_contrib"][0, r, c] == 2
    swapped = _two(3.0, 5.0, swap_index=True)
    for k in ("images", "alpha", "depth", "n_contrib"):
        assert swapped[k].tobytes() == out[k].tobytes(), k
    np.testing.assert_array_equal(swapped["tile_indices"][0, 0, :2], [1, 0])
    np.testing.assert_array_equal(out["tile_indices"][0, 0, :2], [0, 1])
    other = _two(5.0, 3.0)
    img2, _, _ = blend(5.0, 3.0)
    np.testing.assert_allclose(other["images"][0, r, c], img2, rtol=1e-12)
    assert np.max(np.abs(other["images"][0, r, c] - out["images"][0, r, c])) > 0.05


def test_pushforward_off_the_axis_against_a_finite_difference_jacobian():
    """Sigma_px - lowpass I = J_fd Sigma J_fd^T with J_fd the central differences of mu -> project(R mu + t)
    (a primitive inside the tangent clamp)."""
    T_cw = CC.pose((0.3, 1.0, -0.2), 0.4, (0.2, -0.1, 0.3))
    K = (55.0, 62.0, 30.0, 25.0)
    mu = np.array([1.1, -0.6, 4.0])
    rng = np.random.default_rng(9)
    B = rng.normal(size=(3, 3)) * 0.1
    Sig = B @ B.T + 0.01 * np.eye(3)
    s, cond = CS.prep(_one([mu], [Sig], [[1.0, 1.0, 1.0]]), K, T_cw, 48, 64, CS.config())
    assert s["valid"][0] == 1 and cond["clamped"] == 0
    f = lambda m: CS.project(T_cw[:3, :3] @ m + T_cw[:3, 3], K)
    h = 1e-5
    Jfd = np.stack([(f(mu + h * e) - f(mu - h * e)) / (2 * h) for e in np.eye(3)], axis=1)
    want = Jfd @ Sig @ Jfd.T + 0.3 * np.eye(2)
    np.testing.assert_allclose(s["Sigmas_px"][0], want, rtol=1e-8)
    np.testing.assert_allclose(s["Sigmas_inv"][0] @ s["Sigmas_px"][0], np.eye(2), atol=1e-12)
    np.testing.assert_allclose(s["radii"][0], 3.0 * np.sqrt(np.linalg.eigvalsh(s["Sigmas_px"][0])[1]), rtol=1e-13)
    np.testing.assert_allclose(s["means_px"][0], f(mu), rtol=1e-15)
    # at the clamp the Jacobian is the one of the clamped tangent, not of the true one
    far_out = np.linalg.inv(T_cw) @ np.array([4.0 * 3.0, 0.1, 4.0, 1.0])   # x / z = 3 in the camera frame
    s2, cond2 = CS.prep(_one([far_out[:3]], [Sig], [[1.0, 1.0, 1.0]]), K, T_cw, 48, 64, CS.config())
    assert cond2["clamped"] == 1
    lim = 1.3 * max(K[2], 64 - K[2]) / K[0]
    J = np.array([[K[0] / 4.0, 0, -K[0] * lim / 4.0], [0, K[1] / 4.0, -K[1] * (0.1 / 4.0) / 4.0]])
    M = J @ T_cw[:3, :3]
    np.testing.assert_allclose(s2["Sigmas_px"][0], M @ Sig @ M.T + 0.3 * np.eye(2), rtol=1e-10)


def test_camera_from_world_against_a_hand_written_pose(monkeypatch):
    """The body at (1, 2, 3) turned 90 degrees about z; the camera 0.5 m ahead of the body along its x,
    looking along the body's x (optical z), image x to the body's -y, image y to the body's -z."""
    def boom(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_abi, "call", boom)
    monkeypatch.setattr(_abi, "default_context", boom)
    T_wb = np.array([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0], [0.0, 0.0, 0.0, 1.0]])
    np.testing.assert_allclose(R.camera_from_world(T_wb), [[0, 1, 0, -2], [-1, 0, 0, 1], [0, 0, 1, -3], [0, 0, 0, 1]],
                               atol=1e-15)
    R_bc = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    T_cw = R.camera_from_world(T_wb, R_bc, [0.5, 0.0, 0.0])
    # the camera centre in the world: body origin + 0.5 along the body's x, which is the world's y
    np.testing.assert_allclose(-T_cw[:3, :3].T @ T_cw[:3, 3], [1.0, 2.5, 3.0], atol=1e-15)
    # a world point 2 m ahead of the camera along the world's y, 1 m to the world's +x (the body's -y: image +x)
    np.testing.assert_allclose(T_cw @ [2.0, 4.5, 3.0, 1.0], [1.0, 0.0, 2.0, 1.0], atol=1e-15)
    np.testing.assert_allclose(T_cw, CS.camera_from_world(T_wb, R_bc, [0.5, 0.0, 0.0]), atol=1e-15)
    for bad in (np.zeros(5), np.eye(3), np.full(6, np.nan)):
        with pytest.raises(ValueError):
            R.camera_from_world(bad)
    with pytest.raises(ValueError):
        R.camera_from_world(np.eye(4), np.eye(2))
    with pytest.raises(ValueError):
        R.camera_from_world(np.eye(4) * 2.0)   # bottom row (0, 0, 0, 2)


def test_config_defaults():
    c = R.CameraViewConfig()
    d = dataclasses.asdict(c)
    assert d == dict(CS.CFG) and CS.CFG["alpha_skip"] == 1 / 255
    with pytest.raises(Exception):
        c.near = 1.0  # frozen


# ------------------------------------------------------------------ conditions and branches
@pytest.mark.parametrize("name", list(CC.CASES))
def test_case_conditions(name):
    c = CC.build(name)
    out, conds = CC.restated(name)
    cap = c["cfg"]["max_splats_per_tile"]
    for v, cd in enumerate(conds):
        print(name, v, {k: (float("%.3g" % x) if isinstance(x, float) else x) for k, x in cd.items()})
        assert cd["bbox_margin"] >= 1e-9
        assert cd["depth_gap"] >= 1e-9
        assert cd["tie_pairs"] <= {(10, 200)}          # the one deliberate tie, the lower index first
        assert cd["skip_margin"] >= 1e-9 and cd["stop_margin"] >= 1e-9
        assert cd["z_margin"] >= 1e-9
        assert cd["condition"] <= 100.0
        np.testing.assert_array_equal(out["tile_counts"][v], np.minimum(out["tile_survivors"][v], cap))
        assert (out["tile_indices"][v] >= -1).all() and (out["tile_indices"][v] < max(len(out["alphas"]), 1)).all()
    assert out["images"].shape == (len(c["Ks"]), c["H"], c["W"], 3)


def test_cases_reach_their_branches():
    out, conds = CC.restated("cap16")
    busy = out["tile_survivors"][0] > 16
    assert busy.sum() >= 6 and (out["tile_counts"][0][busy] == 16).all() and conds[0]["cut"] == busy.sum()
    assert 20 <= conds[0]["clamped"] <= 40
    out, conds = CC.restated("cap256")
    assert conds[0]["cut"] == 0 and conds[0]["max_survivors"] > 40 and conds[0]["tie_pairs"] == {(10, 200)}
    assert (out["tile_counts"][0] == out["tile_survivors"][0]).all()
    assert CC.build("cap256")["batch"]["mu_world"].shape[0] > 256      # more than one chunk of the selection
    assert not np.array_equal(out["images"], CC.restated("cap16")[0]["images"])
    out, conds = CC.restated("two_views")
    assert out["images"].shape[0] == 2 and np.max(np.abs(out["images"][0] - out["images"][1])) > 0.1
    assert out["valid"].all() and np.max(np.abs(out["colors"][0] - out["colors"][1])) > 1e-3   # the shading moves
    out, conds = CC.restated("invalid")
    bad = list(CC.INVALID_ROWS)
    assert not out["valid"][0, bad].any() and out["valid"][0].sum() == 60 - len(bad)
    assert np.isinf(out["depths"][0, bad]).all() and not out["means_px"][0, bad].any()
    assert not np.isin(out["tile_indices"], bad).any() and np.isfinite(out["images"]).all()
    out, conds = CC.restated("stack")
    assert conds[0]["stopped"] > 100 and out["n_contrib"][0, 24, 32] == 6
    assert set(np.unique(out["n_contrib"])) == {6, 7, 8}
    np.testing.assert_allclose(out["alphas"][:8], 0.8, rtol=1e-15)
    np.testing.assert_array_equal(out["tile_indices"][0, 0, :8], np.arange(8)[::-1])     # back to front by index
    assert 3.0 < out["depth"][0, 24, 32] < 3.3                                           # the front layers dominate
    out, _ = CC.restated("no_shade")
    b = CC.build("no_shade")["batch"]
    assert out["colors"][0].tobytes() == (b["color"] * out["valid"][0][:, None]).tobytes()
    out, _ = CC.restated("background")
    plain, _ = CC.restated("no_shade")
    assert np.array_equal(out["alpha"], plain["alpha"]) and (out["alpha"] < 1e-3).any()
    empty_px = out["n_contrib"][0] == 0
    assert empty_px.any() and (out["images"][0][empty_px] == np.array([0.25, 0.5, 0.75])).all()
    out, conds = CC.restated("one_tile")
    assert out["tile_counts"].shape == (1, 1) and out["tile_counts"][0, 0] > 50
    out, conds = CC.restated("cap1")
    assert out["n_contrib"].max() == 1 and conds[0]["cut"] > 0 and out["tile_indices"].shape[-1] == 1
    out, _ = CC.restated("three_views_ts8")
    assert out["tile_counts"].shape == (3, 16)
    out, _ = CC.restated("empty")
    assert out["alphas"].shape == (0,) and (out["images"] == np.array([0.1, 0.2, 0.3])).all()
    assert not out["alpha"].any() and not out["depth"].any() and (out["tile_indices"] == -1).all()


# --------------------------------------------------------------------------- argument errors
def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_abi, "lib", boom)
    monkeypatch.setattr(_abi, "default_context", boom)
    monkeypatch.setattr(_abi, "call", boom)
    monkeypatch.setattr(_abi, "alloc_many", boom)


def _bad_calls():
    """(what, intrinsics, T_cw, H, W, config overrides) for every argument error of the issue's list."""
    K, I4 = PinholeIntrinsics(*CC.K0), np.eye(4)
    nan, inf = float("nan"), float("inf")
    bottom = np.eye(4)
    bottom[3, 0] = 1e-3
    skew = np.eye(4)
    skew[0, 1] = 1e-6
    scaled = np.eye(4)
    scaled[:3, :3] *= 1.0 + 1e-8
    nanT = np.eye(4)
    nanT[1, 3] = nan
    return [
        ("tile_size 0", K, I4, 48, 64, dict(tile_size=0)), ("tile_size 33", K, I4, 66, 66, dict(tile_size=33)),
        ("tile_size 2.5", K, I4, 50, 50, dict(tile_size=2.5)),
        ("H no multiple", K, I4, 50, 64, {}), ("W no multiple", K, I4, 48, 70, {}), ("H = 0", K, I4, 0, 64, {}),
        ("W too large", K, I4, 48, 16400, {}),
        ("cap 0", K, I4, 48, 64, dict(max_splats_per_tile=0)), ("cap 257", K, I4, 48, 64, dict(max_splats_per_tile=257)),
        ("no view", K, np.zeros((0, 4, 4)), 48, 64, {}), ("33 views", [K] * 33, np.tile(I4, (33, 1, 1)), 48, 64, {}),
        ("T_cw shape", K, np.eye(3), 48, 64, {}),
        ("intrinsics count", [K, K], I4, 48, 64, {}), ("intrinsics count", K, np.tile(I4, (2, 1, 1)), 48, 64, {}),
        ("fx = 0", PinholeIntrinsics(0.0, 60.0, 32.0, 24.0), I4, 48, 64, {}),
        ("fy < 0", PinholeIntrinsics(60.0, -1.0, 32.0, 24.0), I4, 48, 64, {}),
        ("cx NaN", PinholeIntrinsics(60.0, 60.0, nan, 24.0), I4, 48, 64, {}),
        ("fx inf", PinholeIntrinsics(inf, 60.0, 32.0, 24.0), I4, 48, 64, {}),
        ("T_cw NaN", K, nanT, 48, 64, {}), ("bottom row", K, bottom, 48, 64, {}),
        ("no rotation", K, skew, 48, 64, {}), ("scaled rotation", K, scaled, 48, 64, {}),
        ("near 0", K, I4, 48, 64, dict(near=0.0)), ("far = near", K, I4, 48, 64, dict(near=1.0, far=1.0)),
        ("alpha_max 0", K, I4, 48, 64, dict(alpha_max=0.0)), ("alpha_max > 1", K, I4, 48, 64, dict(alpha_max=1.5)),
        ("lowpass NaN", K, I4, 48, 64, dict(lowpass_px2=nan)), ("t_stop inf", K, I4, 48, 64, dict(t_stop=inf)),
        ("background NaN", K, I4, 48, 64, dict(background=(0.0, nan, 0.0))),
        ("background of 2", K, I4, 48, 64, dict(background=(0.0, 0.0))),
    ]


def test_argument_errors_need_no_library(monkeypatch):
    _no_device(monkeypatch)
    b = CC.build("no_shade")["batch"]
    host = R.RenderablePrimitiveBatch(mu_world=b["mu_world"], Sigma_world=b["Sigma_world"], Lambda_world=None,
                                      eta=b["eta"], mass=b["mass"], color=b["color"])
    dev = types.SimpleNamespace(count=120, ctx=None, struct=None)          # stands in for a device batch
    for what, K, T, h, w, over in _bad_calls():
        cfg = R.CameraViewConfig(**over)
        with pytest.raises(ValueError):
            R.render_map_camera(host, K, T, h, w, cfg)
        with pytest.raises(ValueError):
            R.camera_splat_prep(dev, K, T, h, w, cfg)
    K, I4 = PinholeIntrinsics(*CC.K0), np.eye(4)
    with pytest.raises(ValueError):
        R.render_map_camera(object(), K, I4, 48, 64)
    big = types.SimpleNamespace(count=1 << 24, ctx=None, struct=None)
    with pytest.raises(ValueError):
        R.camera_splat_prep(big, K, I4, 16384, 16384)                      # n_views * T * n >= 2^32
    # render_depth_tiles reads the view and splat counts off the splats' shapes
    arr = lambda *shape: types.SimpleNamespace(shape=shape, ctx=None, ptr=None)
    splats = lambda nv, n: dict(means_px=arr(nv, n, 2), Sigmas_inv=arr(nv, n, 2, 2), depths=arr(nv, n), radii=arr(nv, n),
                                alphas=arr(n), colors=arr(nv, n, 3), valid=arr(nv, n))
    C = R.CameraViewConfig
    for h, w, cfg in ((48, 64, C(tile_size=0)), (48, 64, C(tile_size=33)), (50, 64, C()), (48, 70, C()), (0, 64, C()),
                      (48, 16400, C()), (48, 64, C(max_splats_per_tile=0)), (48, 64, C(max_splats_per_tile=257)),
                      (48, 64, C(near=-1.0)), (48, 64, C(far=0.1)), (48, 64, C(alpha_max=0.0)), (48, 64, C(alpha_max=2.0)),
                      (48, 64, C(alpha_skip=float("nan"))), (48, 64, C(eps=float("inf")))):
        with pytest.raises(ValueError):
            R.render_depth_tiles(splats(1, 10), h, w, cfg)
    with pytest.raises(ValueError):
        R.render_depth_tiles(splats(0, 10), 48, 64)
    with pytest.raises(ValueError):
        R.render_depth_tiles(splats(33, 10), 48, 64)
    with pytest.raises(ValueError):
        R.render_depth_tiles(splats(4, 1 << 24), 16384, 16384)
