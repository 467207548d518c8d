"""RGB-D surfel extraction, the CPU side: the preconditions of the GPU comparison for every case
(tests/depth_surfel_cases.py) on the NumPy restatement alone (tests/depth_surfel_restatement.py), properties
of that restatement (a noiseless plane, a uniform colour, the even selection rule), and the operator's
argument errors, which must be raised before any device is touched."""

import numpy as np
import pytest

from gcslam import _abi
from gcslam.measurement_batch import BATCH_ARRAYS
from gcslam.ops import (DepthSurfelConfig, MeasurementBatch, PinholeIntrinsics, create_empty_measurement_batch,
                        extract_depth_surfels)

import depth_surfel_cases as DC
import depth_surfel_restatement as DR


@pytest.mark.parametrize("name", DC.NAMES)
def test_case_preconditions(name):
    r = DC.reference(name)
    s = DC.check_conditions(r)
    c = DC.build(name)
    assert max(c["depth"].shape) <= 96 and c["depth"].shape[0] <= 64
    if name == "planes":
        assert s["n_cells"] == 12 and c["rgb"].std() > 50.0  # textured
    if name == "edge":  # partial cells on both borders: the bottom row is kept, the right column dropped by min_fill
        assert r["cell_n"].tolist()[3::4] == [32, 32, 10] and r["cell_n"].tolist()[8:11] == [80, 80, 80]
        assert r["cell_valid"][8:11].all() and not r["cell_fill_ok"][3::4].any()
    if name == "overflow":  # thinned evenly, not the top rows of the image
        assert s["n_cells"] == 96 and s["valid"] > 13 == s["kept"]
        V = s["valid"]
        want = [c_ for r_, c_ in enumerate(np.flatnonzero(r["cell_valid"])) if (r_ + 1) * 13 // V > r_ * 13 // V]
        assert r["kept_cells"].tolist() == want and r["kept_cells"].max() >= 84
        assert r["rows"].tolist() == list(range(3, 16)) and r["n_camera_valid"] == 16
        np.testing.assert_array_equal(r["slot_cells"][3:], r["kept_cells"])
        assert (r["slot_cells"][:3] == -1).all()
        base = DC.base_arrays(16, 8, 3)
        for k in DR.ARRAYS:  # the rows below n_camera_valid and the LiDAR slice keep the base's values
            np.testing.assert_array_equal(r[k][:3], base[k][:3])
            np.testing.assert_array_equal(r[k][16:], base[k][16:])
    if name in ("grazing", "empty"):
        assert r["n_new"] == 0 and (r["slot_cells"] == -1).all()
        assert not any(r[k].any() for k in DR.ARRAYS)
    if name == "no_rgb":  # the LiDAR rows' grey
        rows = r["rows"]
        np.testing.assert_array_equal(r["colors"][rows, 0], r["colors"][rows, 2])
        np.testing.assert_allclose(r["colors"][rows, 0], 0.25 + 0.25 * (r["cell_normal"][r["kept_cells"], 2] + 1.0), rtol=1e-15)
    if name == "quadratic":
        assert (r["Lambdas"] != DC.reference("planes")["Lambdas"]).any()


def _plane_depth(H, W, K, nrm, off):
    fx, fy, cx, cy = K
    i, j = np.mgrid[0:H, 0:W]
    d = np.stack([(j + 0.5 - cx) / fx, (i + 0.5 - cy) / fy, np.ones((H, W))], axis=-1)
    return off / (d @ nrm)


def test_restatement_noiseless_plane():
    """A noiseless tilted plane n . p_c = off (f64 depths, so no float32 rounding) seen through R, t: every
    cell's normal is R n with n_z >= 0 and its position lies on the plane, to 1e-9."""
    K, H, W = (57.6, 57.6, 32.0, 24.0), 48, 64
    nrm = np.array([0.2, -0.3, 1.0]) / np.linalg.norm([0.2, -0.3, 1.0])
    r = DR.extract(_plane_depth(H, W, K, nrm, 2.0), None, K, DC.R_BC, DC.T_BC, 0.0, dict(n_feat=16, n_surfel=8))
    assert r["n_new"] == 12 and r["rows"].tolist() == list(range(12))
    nb = DC.R_BC @ nrm
    sgn = 1.0 if nb[2] >= 0.0 else -1.0
    nb, off_b = sgn * nb, sgn * (2.0 + nb @ DC.T_BC)  # n_b . p_b = off + n_b . t
    eta0 = r["etas"][r["rows"], 0]
    normals = eta0 / np.linalg.norm(eta0, axis=1, keepdims=True)
    pos = np.linalg.solve(r["Lambdas"][r["rows"]] + 1e-9 * np.eye(3)[None], r["thetas"][r["rows"]][..., None])[..., 0]
    assert np.abs(normals - nb[None]).max() < 1e-9 and np.abs(pos @ nb - off_b).max() < 1e-9
    assert np.abs(r["positions"] @ nb - off_b).max() < 1e-9
    np.testing.assert_array_equal(r["weights"][r["rows"]], 1.0)
    np.testing.assert_array_equal(r["sources"][r["rows"]], 0)
    assert not r["etas"][r["rows"], 1:].any() and r["valid_mask"][r["rows"]].all()


def test_restatement_uniform_colour_is_exact():
    c = DC.build("planes")
    rgb = np.empty(c["depth"].shape + (3,), np.uint8)
    rgb[...] = (200, 17, 101)
    r = DR.extract(c["depth"], rgb, c["K"], c["R"], c["t"], 0.0, c["cfg"])
    assert r["n_new"] > 0
    np.testing.assert_array_equal(r["colors"][r["rows"]], np.broadcast_to(np.array([200, 17, 101]) / 255.0, (r["n_new"], 3)))


def test_selection_keeps_exactly_free():
    for V in range(0, 201):
        for free in range(0, 201):
            kept = DR.select(V, free)
            assert kept.size == min(V, free), (V, free)
            assert kept.size == 0 or ((np.diff(kept) > 0).all() and 0 <= kept[0] and kept[-1] < V)
    # spread evenly: the gaps between kept ranks differ by at most one
    gaps = np.diff(DR.select(96, 13))
    assert gaps.max() - gaps.min() <= 1


def test_config_defaults():
    assert DepthSurfelConfig().__dict__ == dict(DR.DEFAULTS)
    b = create_empty_measurement_batch(4, 8)
    assert b.depth_slot_cells is None and b.lidar_slot_cells is None
    assert isinstance(b, MeasurementBatch)


def test_argument_errors_need_no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device context was requested before the arguments were checked")

    monkeypatch.setattr(_abi, "default_context", no_device)
    monkeypatch.setattr(_abi, "call", no_device)
    K = PinholeIntrinsics(60.0, 60.0, 32.0, 24.0)
    d, rgb = np.ones((48, 64), np.float32), np.zeros((48, 64, 3), np.uint8)
    C = DepthSurfelConfig
    nan = float("nan")
    bad_cfgs = [("cell_px", dict(cell_px=3)), ("cell_px", dict(cell_px=33)), ("cell_px", dict(cell_px=8.5)),
                ("min_fill", dict(min_fill=0.0)), ("min_fill", dict(min_fill=1.5)),
                ("depth limits", dict(min_depth_m=-0.1)), ("depth limits", dict(min_depth_m=2.0, max_depth_m=2.0)),
                ("depth_model", dict(depth_model="cubic")), ("depth_sigma0", dict(depth_sigma0=0.0)),
                ("depth_sigma0", dict(depth_sigma_slope=-1.0)), ("plane_gate", dict(plane_gate=0.0)),
                ("min_cos_incidence", dict(min_cos_incidence=1.0)), ("min_cos_incidence", dict(min_cos_incidence=-0.1)),
                ("n_feat", dict(n_feat=-1)), ("n_surfel", dict(n_surfel=2.5)),
                ("finite", dict(weight_scale=nan)), ("finite", dict(plane_gate=float("inf"))), ("finite", dict(eps_lift=nan))]
    for match, kw in bad_cfgs:
        with pytest.raises(ValueError, match=match):
            extract_depth_surfels(d, rgb, K, config=C(**kw))
    with pytest.raises(ValueError, match="PinholeIntrinsics"):
        extract_depth_surfels(d, rgb, (60.0, 60.0, 32.0, 24.0))
    with pytest.raises(ValueError, match="intrinsics"):
        extract_depth_surfels(d, rgb, PinholeIntrinsics(nan, 60.0, 32.0, 24.0))
    with pytest.raises(ValueError, match="intrinsics"):
        extract_depth_surfels(d, rgb, PinholeIntrinsics(60.0, 0.0, 32.0, 24.0))
    with pytest.raises(ValueError, match=r"expected \(H, W\)"):
        extract_depth_surfels(np.ones(48, np.float32), None, K)
    with pytest.raises(ValueError, match="16384"):
        extract_depth_surfels(np.ones((1, 16385), np.float32), None, K)
    with pytest.raises(ValueError, match="cells"):
        extract_depth_surfels(np.ones((1024, 1024), np.float32), None, K, config=C(cell_px=4))
    with pytest.raises(ValueError, match="rgb"):
        extract_depth_surfels(d, rgb[:, :60], K)
    with pytest.raises(ValueError, match="rgb"):
        extract_depth_surfels(d, rgb[..., 0], K)
    with pytest.raises(ValueError, match="uint8"):
        extract_depth_surfels(d, rgb.astype(np.float32), K)
    with pytest.raises(ValueError, match="expected"):
        extract_depth_surfels(d, rgb, K, R_base_camera=np.eye(4))
    with pytest.raises(ValueError, match="extrinsics must be finite"):
        extract_depth_surfels(d, rgb, K, t_base_camera=[0.0, nan, 0.0])
    with pytest.raises(ValueError, match="extrinsics must be finite"):
        extract_depth_surfels(d, rgb, K, R_base_camera=np.full((3, 3), np.inf))
    with pytest.raises(ValueError, match="timestamp_sec"):
        extract_depth_surfels(d, rgb, K, timestamp_sec=nan)
    with pytest.raises(ValueError, match="base_batch budgets"):
        extract_depth_surfels(d, rgb, K, config=C(n_feat=4, n_surfel=8), base_batch=create_empty_measurement_batch(4, 16))
    base = create_empty_measurement_batch(4, 8)
    base.n_camera_valid = 5
    with pytest.raises(ValueError, match="n_camera_valid"):
        extract_depth_surfels(d, rgb, K, config=C(n_feat=4, n_surfel=8), base_batch=base)
    base = create_empty_measurement_batch(4, 8)
    base.etas = np.zeros((12, 3, 2))
    with pytest.raises(ValueError, match="etas"):
        extract_depth_surfels(d, rgb, K, config=C(n_feat=4, n_surfel=8), base_batch=base)
    assert set(BATCH_ARRAYS) == set(DR.ARRAYS)
