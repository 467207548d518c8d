"""The keypoint detector on the device (csrc/gc_keypoints.hip, gcslam/ops/keypoint_detector.py) against
the restatement (tests/keypoint_restatement.py), bytewise and in stage order, so a failure names its
stage: the grey image, every pyramid level, the three counts per level, meta, and the (u, v, response)
table with its zero tail. No comparison carries a tolerance. The conditions under which the cases pin
an implementation are asserted in test_keypoint_detector.py."""

import numpy as np
import pytest

import keypoint_cases as KC
import keypoint_restatement as KR
from gcslam import _abi
from gcslam.measurement_batch import BATCH_ARRAYS
from gcslam.ops import (DeviceCameraFeatures, DeviceKeypoints, Keypoints, OrbDetectorConfig, PinholeIntrinsics,
                        VisualFeatureConfig, camera_measurement_batch, detect_keypoints, lift_camera_features)


def _run(ctx, image, cfg):
    """One device call: (DeviceKeypoints, [levels on the host], table, meta) with the full arrays."""
    dev, pyr = detect_keypoints(image, cfg, ctx=ctx, device_out=True, return_pyramid=True)
    assert isinstance(dev, DeviceKeypoints)
    return dev, [p.download() for p in pyr], dev.table.download(), dev.meta.download()


def _check(name, got, ref):
    dev, levels, table, meta = got
    L = len(ref["plan"]["sizes"])
    assert levels[0].tobytes() == ref["grey"].tobytes(), f"{name}: grey"
    assert len(levels) == L
    for l in range(1, L):
        assert levels[l].shape == ref["levels"][l].shape and levels[l].tobytes() == ref["levels"][l].tobytes(), \
            f"{name}: pyramid level {l}"
    want = ref["counts"][:3 * L].reshape(L, 3)
    for q, what in enumerate(("after non-maximum suppression", "after the border", "kept")):
        assert dev.counts[:, q].tolist() == want[:, q].tolist(), f"{name}: counts {what}"
    assert dev.count == ref["total"], f"{name}: total"
    assert meta.dtype == np.int32 and meta.tobytes() == ref["meta"].tobytes(), f"{name}: meta"
    assert table.dtype == np.float64 and table.tobytes() == ref["table"].tobytes(), f"{name}: table"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KC.CASES))
def test_gpu_keypoints_equal_restatement(ctx, name):
    """Each case twice from the host image and once from a DeviceArray image: the restatement's bytes,
    and the same bytes all three times."""
    case = KC.build(name)
    cfg = KC.config(name)
    a = _run(ctx, case["image"], cfg)
    _check(name, a, case["ref"])
    b = _run(ctx, case["image"], cfg)
    c = _run(ctx, _abi.DeviceArray.from_host(ctx, case["image"], np.uint8), cfg)
    for other in (b, c):
        assert other[0].count == a[0].count and np.array_equal(other[0].counts, a[0].counts)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(other[1], a[1]))
        assert other[2].tobytes() == a[2].tobytes() and other[3].tobytes() == a[3].tobytes()
    # the host result is the first count rows
    h = detect_keypoints(case["image"], cfg, ctx=ctx)
    ref = case["ref"]
    n = ref["total"]
    assert isinstance(h, Keypoints) and len(h) == n
    assert h.uv.tobytes() == ref["table"][:n, :2].tobytes() and h.response.tobytes() == ref["table"][:n, 2].tobytes()
    assert np.array_equal(h.level, ref["meta"][:n, 0]) and np.array_equal(h.xy_level, ref["meta"][:n, 1:3])
    assert np.array_equal(h.fast_score, ref["meta"][:n, 3]) and np.array_equal(h.counts, a[0].counts)
    hh = a[0].to_host()
    assert hh.uv.tobytes() == h.uv.tobytes() and hh.response.tobytes() == h.response.tobytes()


@pytest.mark.gpu
def test_gpu_keypoints_nothing_carries_over(ctx):
    """flat directly after noise on the same context: zero keypoints and a zero table, so the counters
    and the candidate list start afresh in every call."""
    noise, flat = KC.build("noise"), KC.build("flat")
    a = _run(ctx, noise["image"], KC.config("noise"))
    assert a[0].count == noise["ref"]["total"] > 0
    b = _run(ctx, flat["image"], KC.config("flat"))
    assert b[0].count == 0 and not b[0].counts.any() and not b[2].any() and not b[3].any()
    _check("noise after flat", _run(ctx, noise["image"], KC.config("noise")), noise["ref"])


@pytest.mark.gpu
def test_gpu_keypoints_smallest_images(ctx):
    """Images below one tile and below FAST's 7 x 7 reach: a 1 x 1 image, sixteen levels that all clamp
    to one pixel or so, and a 9 x 9 image with edge_threshold 4, whose one keypoint's Harris block
    touches all four image sides."""
    one = np.array([[200]], np.uint8)
    thin = np.random.default_rng(3).integers(0, 256, (3, 5, 3), dtype=np.uint8)
    dot = np.zeros((9, 9), np.uint8)
    dot[4, 4] = 100
    for name, img, p in (("1x1", one, dict(nfeatures=4, nlevels=1, edge=4)),
                         ("5x3", thin, dict(nfeatures=7, nlevels=16, edge=4)),
                         ("dot", dot, dict(nfeatures=8, nlevels=3, edge=4))):
        ref = KR.detect(img, p["nfeatures"], 1.2, p["nlevels"], p["edge"], 20, 0.04)
        cfg = OrbDetectorConfig(max_features=p["nfeatures"], n_levels=p["nlevels"], edge_threshold=p["edge"])
        _check(name, _run(ctx, img, cfg), ref)
    assert ref["total"] >= 1 and ref["meta"][0].tolist() == [0, 4, 4, 99]


@pytest.mark.gpu
def test_gpu_keypoints_device_chain(ctx):
    """rgb8 + depth -> detect_keypoints(device_out) -> lift_camera_features(device_out) ->
    camera_measurement_batch, nothing but the counters returning to the host, gives the bytes of the same
    chain with the keypoints downloaded and passed as host arrays."""
    import camsplat_cases as CC
    depth, rgb = KC.scene()
    intr = PinholeIntrinsics(*KC.SCENE_K)
    det = OrbDetectorConfig(max_features=64, n_levels=4)
    vcfg = VisualFeatureConfig(max_features=64)
    points = CC.build("mixed")["points_base"]
    d_rgb = _abi.DeviceArray.from_host(ctx, rgb, np.uint8)
    d_depth = _abi.DeviceArray.from_host(ctx, depth, np.float32)

    def batch(features):
        return camera_measurement_batch(points, features, intr, CC.R_BASE_CAMERA, CC.T_BASE_CAMERA, CC.TIMESTAMP,
                                        n_feat=64, n_surfel=64, eps_lift=CC.EPS_LIFT, ctx=ctx, device_out=True)

    kp = detect_keypoints(d_rgb, det, ctx=ctx, device_out=True)
    ref = KR.detect(rgb, 64, 1.2, 4, 31, 20, 0.04)
    assert kp.count == ref["total"] > 16 and kp.table.download().tobytes() == ref["table"].tobytes()
    f_dev = lift_camera_features(d_depth, d_rgb, kp, None, intr, vcfg, ctx=ctx, device_out=True)
    assert isinstance(f_dev, DeviceCameraFeatures) and len(f_dev) == kp.count
    host = kp.to_host()
    f_host = lift_camera_features(depth, rgb, host.uv, host.response, intr, vcfg, ctx=ctx)
    assert len(f_host) == kp.count and f_host.weight.any()
    a, b = batch(f_dev), batch(f_host)
    for k in BATCH_ARRAYS:
        x, y = a.device[k].download(), b.device[k].download()
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert a.device["weights"].download()[:kp.count].tobytes() == f_host.weight.tobytes()
    # a budget below the count is refused; an empty table gives the empty features
    with pytest.raises(ValueError):
        lift_camera_features(d_depth, d_rgb, kp, None, intr, VisualFeatureConfig(max_features=kp.count - 1), ctx=ctx)
    none = detect_keypoints(KC.image("flat"), det, ctx=ctx, device_out=True)
    assert none.count == 0 and len(lift_camera_features(d_depth, d_rgb, none, None, intr, vcfg, ctx=ctx)) == 0


@pytest.mark.gpu
def test_gpu_keypoints_entry_checks(ctx):
    """gc_keypoints_detect's own argument checks, before any launch; the context stays usable."""
    img = _abi.DeviceArray(ctx, (8, 8, 3), np.uint8)
    out = _abi.DeviceArray(ctx, (4096 * 8,), np.float64)
    base = [16, 1.2, 2, 4, 20, 0.04]

    def call(H=8, W=8, ch=3, cfg=base, image=img.ptr, kp=out.ptr):
        h = np.array(cfg, np.float64)
        _abi.call("gc_keypoints_detect", ctx.handle, H, W, ch, image, h.ctypes.data, out.ptr, kp, out.ptr, out.ptr, ctx=ctx)

    def with_(i, v):
        c = list(base)
        c[i] = v
        return c

    for bad in (dict(H=0), dict(W=0), dict(H=8192, W=8193), dict(ch=2), dict(ch=4), dict(cfg=with_(0, 0)),
                dict(cfg=with_(0, 4097)), dict(cfg=with_(2, 0)), dict(cfg=with_(2, 17)), dict(cfg=with_(1, 1.0)),
                dict(cfg=with_(1, float("inf"))), dict(cfg=with_(1, float("nan"))), dict(cfg=with_(4, 0)),
                dict(cfg=with_(4, 255)), dict(cfg=with_(3, 3)), dict(cfg=with_(3, 1025)), dict(cfg=with_(5, float("nan"))),
                dict(image=None), dict(kp=None)):
        with pytest.raises(ValueError):
            call(**bad)
    case = KC.build("grey_noise")
    _check("grey_noise", _run(ctx, case["image"], KC.config("grey_noise")), case["ref"])
