"""The keypoint detector on the GPU: the detector half of the ORB the reference's visual_feature_node
runs (src/visual_feature_node.cpp:149-158, :512-535: cv::ORB with nfeatures = max_features, scaleFactor
1.2, nlevels 8, edgeThreshold 31, firstLevel 0, HARRIS_SCORE, fastThreshold 20), from the colour image to
a (u, v, response) table in HBM that lift_camera_features reads in place.

It is build-defined: grey conversion, an 8-level bilinear pyramid, FAST-9/16 with the arc score, strict
3 x 3 non-maximum suppression, the border, ORB's per-level quotas with a first cut by FAST score and a
second by Harris response (DESIGN.md §4 "Keypoint detector" states every step). It follows the
published algorithms and was not checked against OpenCV; it does not claim OpenCV's bits, and it
computes no angle, size or descriptor (nothing downstream reads them). All arithmetic runs in libgcslam
(csrc/gc_keypoints.hip), integer but for seven f64 operations per response, so results are bitwise
reproducible; every argument error is raised here before a device is asked for."""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from .. import _abi

MAX_PIXELS = _abi.GC_IMAGE_MAX_PIXELS


@dataclass(frozen=True)
class OrbDetectorConfig:
    """The arguments the node gives cv::ORB::create (visual_feature_node.cpp:149-158) and Harris's k.
    They are the members of gc_kp_cfg (include/gcslam.h); max_features and n_levels are ORB's nfeatures and
    nlevels there."""
    max_features: int = 512
    scale_factor: float = 1.2
    n_levels: int = 8
    edge_threshold: int = 31
    fast_threshold: int = 20
    harris_k: float = 0.04


@dataclass
class Keypoints:
    """The M keypoints of one image on the host, levels ascending, inside a level by descending
    response then ascending raster index. uv is in level-0 pixels (x s_l, y s_l); xy_level the integer
    position on the keypoint's own level; counts (n_levels, 3) the corners of each level after
    non-maximum suppression, after the border, and kept."""
    uv: np.ndarray          # (M, 2) float64
    response: np.ndarray    # (M,) float64
    level: np.ndarray       # (M,) int32
    xy_level: np.ndarray    # (M, 2) int32
    fast_score: np.ndarray  # (M,) int32
    counts: np.ndarray      # (n_levels, 3) int32

    def __len__(self) -> int:
        return int(self.uv.shape[0])


@dataclass
class DeviceKeypoints:
    """The detector's tables in HBM, as detect_keypoints(..., device_out=True) leaves them: table
    (max_features, 3) = (u, v, response) float64 and meta (max_features, 4) = (level, x, y, FAST score)
    int32, rows from count on zero. count and counts are on the host: they came with the call's one small
    download. lift_camera_features takes a DeviceKeypoints as its keypoints_uv and reads the first count
    rows of table where they are."""
    table: "_abi.DeviceArray"
    meta: "_abi.DeviceArray"
    count: int
    counts: np.ndarray      # (n_levels, 3) int32

    def __len__(self) -> int:
        return int(self.count)

    def to_host(self) -> Keypoints:
        t, m = _abi.download_many([self.table, self.meta])
        n = self.count
        return Keypoints(uv=np.ascontiguousarray(t[:n, :2]), response=np.ascontiguousarray(t[:n, 2]),
                         level=np.ascontiguousarray(m[:n, 0]), xy_level=np.ascontiguousarray(m[:n, 1:3]),
                         fast_score=np.ascontiguousarray(m[:n, 3]), counts=self.counts.copy())


def _int_in(v, lo: int, hi: int, what: str) -> int:
    try:
        ok = math.isfinite(v) and int(v) == v and lo <= v <= hi
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what} must be an integer in [{lo}, {hi}], got {v!r}")
    return int(v)


def _cfg(cfg: OrbDetectorConfig):
    """gc_kp_cfg (include/gcslam.h), checked as the device entry checks it."""
    try:
        k = _int_in(cfg.max_features, 1, _abi.GC_CAM_MAX_QUERIES, "max_features")
        levels = _int_in(cfg.n_levels, 1, _abi.GC_KP_MAX_LEVELS, "n_levels")
        edge = _int_in(cfg.edge_threshold, 4, 1024, "edge_threshold")
        thr = _int_in(cfg.fast_threshold, 1, 254, "fast_threshold")
        sf, hk = float(cfg.scale_factor), float(cfg.harris_k)
    except (TypeError, AttributeError) as e:
        raise ValueError(f"config does not hold the OrbDetectorConfig fields: {e}") from None
    if not (abs(sf) <= 3.40282347e38 and float(np.float32(sf)) > 1.0):  # false for NaN
        raise ValueError(f"scale_factor must be finite and > 1 as float32, got {sf}")
    if not math.isfinite(hk):
        raise ValueError(f"harris_k must be finite, got {hk}")
    return _abi.cfg("gc_kp_cfg", dict(nfeatures=k, scale_factor=sf, nlevels=levels, edge_threshold=edge,
                                      fast_threshold=thr, harris_k=hk))


def _image_shape(image):
    sh = tuple(int(v) for v in (image.shape if isinstance(image, _abi.DeviceArray) else np.shape(image)))
    if len(sh) not in (2, 3) or (len(sh) == 3 and sh[2] != 3):
        raise ValueError(f"image of shape {sh}, expected (H, W, 3) or (H, W)")
    H, W = sh[:2]
    if H < 1 or W < 1 or H * W > MAX_PIXELS:
        raise ValueError(f"an image of {H} x {W}; H and W must be >= 1 and H W <= 2^26")
    return H, W, (3 if len(sh) == 3 else 1)


def keypoints_plan(H: int, W: int, config: Optional[OrbDetectorConfig] = None) -> dict:
    """gc_keypoints_plan (host only): sizes [(W_l, H_l)], scales, quotas, capacities, the levels' byte
    offsets in the pyramid, pyramid_bytes and workspace_bytes."""
    cfg = config or OrbDetectorConfig()
    c_cfg = _cfg(cfg)
    if int(H) != H or int(W) != W or H < 1 or W < 1 or H * W > MAX_PIXELS:
        raise ValueError(f"an image of {H} x {W}; H and W must be integers >= 1 and H W <= 2^26")
    lv = np.zeros((_abi.GC_KP_MAX_LEVELS, _abi.GC_KP_PLAN_ROW), np.int64)
    sc = np.zeros(_abi.GC_KP_MAX_LEVELS, np.float64)
    nb = np.zeros(2, np.int64)
    _abi.call("gc_keypoints_plan", int(H), int(W), C.byref(c_cfg), lv.ctypes.data, sc.ctypes.data, nb.ctypes.data)
    n = int(cfg.n_levels)
    return dict(sizes=[(int(r[0]), int(r[1])) for r in lv[:n]], scales=[float(s) for s in sc[:n]],
                quotas=[int(r[2]) for r in lv[:n]], caps=[int(r[3]) for r in lv[:n]],
                offsets=[int(r[4]) for r in lv[:n]], pyramid_bytes=int(nb[0]), workspace_bytes=int(nb[1]))


def resize_table(n_src: int, n_dst: int):
    """gc_keypoints_resize_table (host only): (i0, w1) int32 of one axis of the pyramid's resize."""
    if int(n_src) != n_src or int(n_dst) != n_dst or not (1 <= n_src <= MAX_PIXELS and 1 <= n_dst <= MAX_PIXELS):
        raise ValueError(f"n_src and n_dst must be integers in [1, 2^26], got {n_src}, {n_dst}")
    i0, w1 = np.zeros(int(n_dst), np.int32), np.zeros(int(n_dst), np.int32)
    _abi.call("gc_keypoints_resize_table", int(n_src), int(n_dst), i0.ctypes.data, w1.ctypes.data)
    return i0, w1


def detect_keypoints(image, config: Optional[OrbDetectorConfig] = None, *, ctx=None, device_out: bool = False,
                     return_pyramid: bool = False):
    """The keypoints of image, a host array or DeviceArray of uint8 and shape (H, W, 3) (rgb8) or (H, W)
    (grey already), by the build-defined detector of DESIGN.md §4 "Keypoint detector" (the detector half
    of visual_feature_node.cpp:149-158, :512-535; not OpenCV's bits). At most config.max_features of
    them, split over the levels by ORB's quotas; a quota a level does not fill is not redistributed.

    Returns Keypoints on the host. With device_out a DeviceKeypoints: the (max_features, 3) table stays
    in HBM for lift_camera_features, and its count arrives with one download of the GC_KP_COUNTS_LEN
    counters (196 B). That download is the call's only wait, as gc_pipeline_get_front_hyp0's is the
    front's: everything before it is enqueued without one. With return_pyramid the second result is the
    list of the levels, level 0 the grey image: host (H_l, W_l) uint8 arrays, or with device_out
    DeviceArray views of the one pyramid buffer."""
    cfg = config or OrbDetectorConfig()
    c_cfg = _cfg(cfg)
    H, W, channels = _image_shape(image)
    if isinstance(image, _abi.DeviceArray):
        if image.dtype != np.uint8:
            raise ValueError(f"device image of dtype {image.dtype}, expected uint8")
    else:
        image = np.asarray(image)
        if image.dtype != np.uint8:
            raise ValueError(f"image of dtype {image.dtype}, expected uint8 (rgb8 or mono8)")
    plan = keypoints_plan(H, W, cfg)
    k, n_levels = int(cfg.max_features), int(cfg.n_levels)
    if ctx is None:
        ctx = image.ctx if isinstance(image, _abi.DeviceArray) else _abi.default_context()
    d_img = _abi.device_input(ctx, image, np.uint8, (H, W, 3) if channels == 3 else (H, W))
    d_pyr = _abi.DeviceArray(ctx, (plan["pyramid_bytes"],), np.uint8)
    d_kp, d_meta, d_counts = _abi.alloc_many(ctx, [((k, 3), np.float64), ((k, 4), np.int32),
                                                   ((_abi.GC_KP_COUNTS_LEN,), np.int32)])
    _abi.call("gc_keypoints_detect", ctx.handle, H, W, channels, d_img.ptr, C.byref(c_cfg), d_pyr.ptr, d_kp.ptr,
              d_meta.ptr, d_counts.ptr, ctx=ctx)
    if device_out:
        c = d_counts.download()
        res = DeviceKeypoints(table=d_kp, meta=d_meta, count=int(c[-1]),
                              counts=np.ascontiguousarray(c[:3 * n_levels].reshape(n_levels, 3)))
    else:
        t, m, c = _abi.download_many([d_kp, d_meta, d_counts])   # one block: one copy
        n = int(c[-1])
        res = Keypoints(uv=np.ascontiguousarray(t[:n, :2]), response=np.ascontiguousarray(t[:n, 2]),
                        level=np.ascontiguousarray(m[:n, 0]), xy_level=np.ascontiguousarray(m[:n, 1:3]),
                        fast_score=np.ascontiguousarray(m[:n, 3]),
                        counts=np.ascontiguousarray(c[:3 * n_levels].reshape(n_levels, 3)))
    if not return_pyramid:
        return res
    views: List = []
    for (w_l, h_l), off in zip(plan["sizes"], plan["offsets"]):
        views.append(_abi.DeviceArray(ctx, (h_l, w_l), np.uint8, _base=d_pyr, _ptr=d_pyr.ptr + off))
    if device_out:
        return res, views
    raw = d_pyr.download()
    return res, [raw[off:off + w_l * h_l].reshape(h_l, w_l).copy() for (w_l, h_l), off in zip(plan["sizes"], plan["offsets"])]
