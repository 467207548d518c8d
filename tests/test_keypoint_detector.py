"""The keypoint detector without a GPU: the restatement (tests/keypoint_restatement.py) held to closed
forms, the library's host entries (gc_keypoints_plan, gc_keypoints_resize_table) held to the
restatement, the conditions under which the cases (tests/keypoint_cases.py) pin an implementation, and
every argument error of detect_keypoints raised before a device is asked for. Nothing here carries a
tolerance: every stage is integer arithmetic or a fixed sequence of f64 operations."""

import dataclasses

import numpy as np
import pytest

import keypoint_cases as KC
import keypoint_restatement as KR
from gcslam import _abi
from gcslam.ops import (DeviceKeypoints, OrbDetectorConfig, VisualFeatureConfig, detect_keypoints,
                        lift_camera_features)
from gcslam.ops import keypoint_detector as KD


# ---- grey
def test_grey_closed_forms():
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]]], np.uint8)
    assert KR.grey(px).tolist() == [[76, 150, 29, 255, 0]]
    g = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert KR.grey(g).tobytes() == g.tobytes()      # an (H, W) image is grey already


# ---- plan
def test_plan_defaults_640x480():
    pl = KR.plan(480, 640)
    assert pl["quotas"] == [111, 93, 77, 64, 54, 45, 37, 31] and sum(pl["quotas"]) == 512
    assert pl["sizes"] == [(640, 480), (533, 400), (444, 333), (370, 278), (309, 231), (257, 193), (214, 161),
                           (179, 134)]
    assert pl["scales"][0] == 1.0 and pl["scales"][1] == float(np.float32(1.2))
    assert KR.plan(150, 200, 64, 1.2, 4)["quotas"] == [21, 17, 14, 12]
    assert KR.plan(10, 10, 7, 1.5, 1)["quotas"] == [7]


@pytest.mark.parametrize("H,W,k,sf,levels", [(480, 640, 512, 1.2, 8), (150, 200, 64, 1.2, 4), (149, 203, 64, 1.2, 4),
                                             (97, 131, 4096, 1.2, 3), (72, 96, 32, 1.2, 2), (5, 3, 1, 1.2, 16),
                                             (1, 1, 9, 2.0, 5), (33, 1000, 100, 1.05, 16), (59, 67, 16, 1.2, 2)])
def test_library_plan_equals_restatement(H, W, k, sf, levels):
    cfg = OrbDetectorConfig(max_features=k, scale_factor=sf, n_levels=levels)
    got, ref = KD.keypoints_plan(H, W, cfg), KR.plan(H, W, k, sf, levels)
    for key in ("sizes", "quotas", "caps"):
        assert got[key] == ref[key], key
    assert np.array(got["scales"]).tobytes() == np.array(ref["scales"]).tobytes()
    # the pyramid: level after level, each on a 256-byte boundary
    off = 0
    for (w, h), o in zip(got["sizes"], got["offsets"]):
        assert o == off and o % 256 == 0
        off += -(-(w * h) // 256) * 256
    assert got["pyramid_bytes"] == off and got["workspace_bytes"] >= 16 * sum(got["caps"])


# ---- resize
def test_resize_closed_forms():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (12, 18), dtype=np.uint8)
    assert KR.resize(a, 18, 12).tobytes() == a.tobytes()                       # same size: the identity
    assert (KR.resize(np.full((9, 13), 77, np.uint8), 11, 7) == 77).all()      # a constant stays constant
    s = a.astype(np.int32)
    half = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
    assert np.array_equal(KR.resize(a, 9, 6), half.astype(np.uint8))           # exact halving
    i0, w1 = KR.resize_table(10, 7)
    assert i0.min() >= 0 and i0.max() <= 9 and w1.min() >= 0 and w1.max() <= 2048
    i0, w1 = KR.resize_table(4, 9)                                             # upsampling clamps both ends
    assert (i0[0], w1[0]) == (0, 0) and (i0[-1], w1[-1]) == (3, 0)


def test_library_resize_table_equals_restatement():
    pairs = {(1, 1), (1, 5), (5, 1), (4, 9), (640, 533)}
    for name in KC.CASES:
        sizes = KC.build(name)["ref"]["plan"]["sizes"]
        for (ws, hs), (wd, hd) in zip(sizes, sizes[1:]):
            pairs |= {(ws, wd), (hs, hd)}
    for n_s, n_d in sorted(pairs):
        got, ref = KD.resize_table(n_s, n_d), KR.resize_table(n_s, n_d)
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes(), (n_s, n_d)
    for bad in ((0, 4), (4, 0), ((1 << 26) + 1, 4)):
        with pytest.raises(ValueError):
            KD.resize_table(*bad)
        with pytest.raises(ValueError):
            buf = np.zeros(8, np.int32)
            _abi.call("gc_keypoints_resize_table", bad[0], bad[1], buf.ctypes.data, buf.ctypes.data)


# ---- FAST and the suppression
def test_fast_single_pixel():
    img = np.zeros((15, 17), np.uint8)
    img[7, 8] = 100
    sc = KR.fast_scores(img, 20)
    assert sc[7, 8] == 99 and np.count_nonzero(sc) == 1     # the whole circle is 100 darker; none around it
    assert np.argwhere(KR.nms(sc)).tolist() == [[7, 8]]


@pytest.mark.parametrize("t", [1, 20, 254])
def test_fast_threshold_is_strict(t):
    img = np.zeros((9, 9), np.uint8)
    img[4, 4] = t
    assert not KR.fast_scores(img, t).any()                 # contrast t: no corner
    img[4, 4] = t + 1
    sc = KR.fast_scores(img, t)
    assert sc[4, 4] == t and np.count_nonzero(sc) == 1      # contrast t + 1: a corner of score t
    dark = np.full((9, 9), 255, np.uint8)
    dark[4, 4] = 255 - (t + 1)
    assert KR.fast_scores(dark, t)[4, 4] == t


def test_ideal_corner_vanishes_in_ties():
    img = np.full((40, 40), 30, np.uint8)
    img[20:, 20:] = 220                                      # a quarter plane
    sc = KR.fast_scores(img, 20)
    assert sc.any() and not KR.nms(sc).any()


def test_nms_survivors_are_never_adjacent():
    for name in ("noise", "periodic"):
        r = KC.build(name)["ref"]
        for sc in r["scores"]:
            keep = KR.nms(sc)
            assert not (keep[:, 1:] & keep[:, :-1]).any() and not (keep[1:] & keep[:-1]).any()
            assert not (keep[1:, 1:] & keep[:-1, :-1]).any() and not (keep[1:, :-1] & keep[:-1, 1:]).any()


# ---- Harris
@pytest.mark.parametrize("alpha,beta", [(1, 0), (0, 2), (3, -2), (-4, 5)])
def test_harris_on_a_ramp(alpha, beta):
    y, x = np.mgrid[0:21, 0:21]
    img = (100 + alpha * (x - 10) + beta * (y - 10)).astype(np.uint8)
    a, b, c = KR.harris_sums(img, [10], [10])
    assert (int(a[0]), int(b[0]), int(c[0])) == (3136 * alpha * alpha, 3136 * beta * beta, 3136 * alpha * beta)
    k = 0.04
    s = float(a[0] + b[0])
    want = (0.0 - k * (s * s)) * KR.harris_scale()           # a b = c c for a ramp
    assert KR.harris_tail(a, b, c, k)[0] == want
    q = 1.0 / 7140.0
    assert KR.harris_scale() == (q * q) * (q * q)


# ---- the cases
@pytest.mark.parametrize("name", list(KC.CASES))
def test_case_within_capacity(name):
    r = KC.build(name)["ref"]
    L = len(r["plan"]["sizes"])
    counts = r["counts"][:3 * L].reshape(L, 3)
    assert (counts[:, 0] <= np.array(r["plan"]["caps"])).all()
    assert (counts[:, 1] <= counts[:, 0]).all() and (counts[:, 2] <= counts[:, 1]).all()
    assert r["total"] == counts[:, 2].sum() == r["counts"][-1] <= KC.CASES[name]["nfeatures"]
    assert not r["table"][r["total"]:].any() and not r["meta"][r["total"]:].any()
    # rows: levels ascending, inside a level descending response then ascending raster index
    m = r["meta"][:r["total"]]
    assert (np.diff(m[:, 0]) >= 0).all()
    for l in range(L):
        rows = np.nonzero(m[:, 0] == l)[0]
        resp = r["table"][rows, 2]
        ras = m[rows, 2].astype(np.int64) * r["plan"]["sizes"][l][0] + m[rows, 1]
        assert all(resp[i] > resp[i + 1] or (resp[i] == resp[i + 1] and ras[i] < ras[i + 1]) for i in range(len(rows) - 1))


def _branches(name):
    r = KC.build(name)["ref"]
    out = set()
    for l, n in enumerate(r["plan"]["quotas"]):
        cand, c1, c2 = r["cands"][l], r["cut1"][l], r["cut2"][l]
        if cand["score"].shape[0] > 2 * n:
            s = np.sort(cand["score"])[::-1]
            out.add("first_cut")
            if s[2 * n - 1] == s[2 * n]:
                out.add("first_cut_tie")
        if c1["x"].shape[0] > n:
            rr = np.sort(c1["response"])[::-1]
            out.add("second_cut")
            if rr[n - 1] == rr[n]:
                out.add("second_cut_tie")
        if c2["x"].shape[0] < n:
            out.add("unfilled")
        W_l, H_l = r["plan"]["sizes"][l]
        e = KC.CASES[name]["edge"]
        if (W_l <= 2 * e or H_l <= 2 * e) and r["counts"][3 * l] > 0 and r["counts"][3 * l + 1] == 0:
            out.add("emptied_by_border")
    if r["total"] == 0:
        out.add("zero")
    return out


def test_cases_reach_every_branch():
    b = {name: _branches(name) for name in KC.CASES}
    assert {"first_cut", "first_cut_tie", "second_cut"} <= b["noise"]
    assert {"first_cut", "second_cut"} <= b["blocks"]
    assert "second_cut_tie" in b["periodic"]
    assert b["noise_unfilled"] == {"unfilled"}               # no cut is active, every quota is unfilled
    assert "emptied_by_border" in b["noise_small"]
    assert b["flat"] == {"zero", "unfilled"}
    # the counts the cases were chosen by
    r = KC.build("noise")["ref"]
    assert r["counts"][[1, 4, 7, 10]].tolist() == [1126, 534, 206, 52] and r["plan"]["quotas"] == [21, 17, 14, 12]
    assert KC.build("noise_unfilled")["ref"]["counts"][[1, 4, 7]].tolist() == [890, 496, 232]
    # an image with one channel goes the same way as its three equal channels would not: it is taken as grey
    g = KC.build("grey_noise")
    assert g["image"].ndim == 2 and g["ref"]["grey"].tobytes() == g["image"].tobytes() and g["ref"]["total"] > 0


# ---- the arguments, before any device
def _bad_configs():
    d = OrbDetectorConfig()
    r = lambda **kw: dataclasses.replace(d, **kw)
    return [r(max_features=0), r(max_features=4097), r(max_features=12.5), r(n_levels=0), r(n_levels=17),
            r(scale_factor=1.0), r(scale_factor=0.5), r(scale_factor=float("nan")), r(scale_factor=float("inf")),
            r(scale_factor=1.0 + 1e-9), r(fast_threshold=0), r(fast_threshold=255), r(edge_threshold=3),
            r(edge_threshold=1025), r(harris_k=float("nan")), r(harris_k=float("inf")), r(max_features="many")]


def test_argument_errors_need_no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(_abi, "default_context", no_device)
    img = KC.image("noise")
    for cfg in _bad_configs():
        with pytest.raises(ValueError):
            detect_keypoints(img, cfg)
        with pytest.raises(ValueError):
            KD.keypoints_plan(150, 200, cfg)
    for bad in (np.zeros((0, 5, 3), np.uint8), np.zeros((5, 0), np.uint8), np.zeros((4, 4, 4), np.uint8),
                np.zeros((4, 4, 1), np.uint8), np.zeros((16,), np.uint8), np.zeros((4, 4, 3), np.float32),
                np.zeros((4, 4), np.int16), np.broadcast_to(np.uint8(0), (8192, 8193))):
        with pytest.raises(ValueError):
            detect_keypoints(bad)
    # the entry's own checks of the plan (host only)
    buf = np.zeros(16 * 5 + 16 + 2, np.int64)
    for H, W, cfg in ((0, 4, None), (4, 0, None), (8192, 8193, None), (4, 4, [0, 1.2, 8, 31, 20, 0.04]),
                      (4, 4, [512, 1.2, 8, 31, 20, float("nan")]), (4, 4, [512, 1.2, 8.5, 31, 20, 0.04]),
                      (4, 4, [512, 1e300, 8, 31, 20, 0.04]), (4, 4, [512, 1.2, 8, 31, 255, 0.04])):
        h = np.array(cfg if cfg is not None else [512, 1.2, 8, 31, 20, 0.04], np.float64)
        with pytest.raises(ValueError):
            _abi.call("gc_keypoints_plan", H, W, h.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data)
    # lift_camera_features and a DeviceKeypoints: the budget, the responses, the empty table
    depth = np.ones((8, 8), np.float32)
    table = _abi.DeviceArray.__new__(_abi.DeviceArray)       # never touched: no device here
    table.shape, table.dtype, table.ptr, table._base, table.ctx = (64, 3), np.dtype(np.float64), None, None, None
    kp = DeviceKeypoints(table=table, meta=None, count=40, counts=np.zeros((1, 3), np.int32))
    with pytest.raises(ValueError, match="max_features"):
        lift_camera_features(depth, None, kp, None, (10.0, 10.0, 4.0, 4.0), VisualFeatureConfig(max_features=32))
    with pytest.raises(ValueError, match="responses"):
        lift_camera_features(depth, None, kp, np.zeros(40), (10.0, 10.0, 4.0, 4.0))
    kp.count = 0
    f = lift_camera_features(depth, None, kp, None, (10.0, 10.0, 4.0, 4.0))
    assert len(f) == 0 and f.cov_xyz.shape == (0, 3, 3)
