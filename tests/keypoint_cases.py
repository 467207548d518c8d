"""TEST INFRASTRUCTURE — the cases of the keypoint-detector tests (test_keypoint_detector.py,
test_gpu_keypoint_detector.py). Everything is drawn from fixed seeds. A case is an image, the detector's
parameters and the restatement's result for them (keypoint_restatement.detect), computed once per process.

  noise           uniform rgb noise: far more corners than 2 n_l on every level, so the first cut is
                  active and a run of equal FAST scores straddles it
  blocks          random rectangles plus +-6 noise: both cuts active, no ties
  periodic        one 25 x 25 tile of two rectangles and +-8 noise repeated: equal responses, a tie at the
                  second cut
  noise_unfilled  noise with a quota no level fills
  noise_small     noise on an image whose level 1 has no interior inside the border
  grey_noise      a one-channel image
  flat            grey 128: no keypoint

The conditions each case must meet are asserted in test_keypoint_detector.py."""

from __future__ import annotations

import numpy as np

import keypoint_restatement as KR

# W, H, nlevels, nfeatures, edge; fast_threshold 20, scale_factor 1.2 and harris_k 0.04 throughout
CASES = {
    "noise": dict(gen="noise", W=200, H=150, nlevels=4, nfeatures=64, edge=31),
    "blocks": dict(gen="blocks", W=200, H=150, nlevels=4, nfeatures=64, edge=31),
    "periodic": dict(gen="periodic", W=203, H=149, nlevels=4, nfeatures=64, edge=16),
    "noise_unfilled": dict(gen="noise", W=131, H=97, nlevels=3, nfeatures=4096, edge=8),
    "noise_small": dict(gen="noise", W=96, H=72, nlevels=2, nfeatures=32, edge=31),
    "grey_noise": dict(gen="grey_noise", W=67, H=59, nlevels=2, nfeatures=16, edge=8),
    "flat": dict(gen="flat", W=200, H=150, nlevels=4, nfeatures=64, edge=31),
}
SCALE_FACTOR, FAST_THRESHOLD, HARRIS_K = 1.2, 20, 0.04


def _noise(W, H):
    return np.random.default_rng(41).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _grey_noise(W, H):
    return np.random.default_rng(45).integers(0, 256, (H, W), dtype=np.uint8)


def _blocks(W, H):
    rng = np.random.default_rng(43)
    img = np.full((H, W, 3), 110, np.int32)
    for _ in range(int(round(60 * W * H / 30000.0))):   # 60 at 200 x 150
        x0, y0 = int(rng.integers(0, W - 8)), int(rng.integers(0, H - 8))
        w, h = int(rng.integers(6, 40)), int(rng.integers(6, 40))
        img[y0:y0 + h, x0:x0 + w] = rng.integers(20, 236, 3)
    img += rng.integers(-6, 7, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def _periodic(W, H):
    tile = np.full((25, 25), 60, np.int32)
    tile[4:13, 5:16] = 200
    tile[10:21, 12:22] = 130
    tile += np.random.default_rng(47).integers(-8, 9, (25, 25))   # ideal corners tie and vanish (step 5)
    tile = tile.astype(np.uint8)
    reps = np.tile(tile, (H // 25 + 1, W // 25 + 1))[:H, :W]
    return np.repeat(reps[:, :, None], 3, axis=2).copy()


def _flat(W, H):
    return np.full((H, W), 128, np.uint8)


_GEN = dict(noise=_noise, grey_noise=_grey_noise, blocks=_blocks, periodic=_periodic, flat=_flat)


def image(name):
    c = CASES[name]
    return _GEN[c["gen"]](c["W"], c["H"])


def params(name):
    c = CASES[name]
    return dict(nfeatures=c["nfeatures"], scale_factor=SCALE_FACTOR, nlevels=c["nlevels"], edge=c["edge"],
                fast_threshold=FAST_THRESHOLD, harris_k=HARRIS_K)


def config(name):
    from gcslam.ops import OrbDetectorConfig
    p = params(name)
    return OrbDetectorConfig(max_features=p["nfeatures"], scale_factor=p["scale_factor"], n_levels=p["nlevels"],
                             edge_threshold=p["edge"], fast_threshold=p["fast_threshold"], harris_k=p["harris_k"])


_cache = {}


def build(name):
    """The case's image, parameters and the restatement's result (shared, not to be changed)."""
    if name not in _cache:
        img = image(name)
        _cache[name] = dict(name=name, image=img, params=params(name), ref=KR.detect(img, **params(name)))
    return _cache[name]


# ---- the scene of the chain test: camfeat_cases' depth regions at another image size, and a colour
# image with corners on it
SCENE_W, SCENE_H = 200, 150
SCENE_K = (160.0, 160.0, 100.0, 75.0)   # fx, fy, cx, cy


def scene(W=SCENE_W, H=SCENE_H, K=SCENE_K, seed=41):
    """(depth float32 (H, W), rgb uint8 (H, W, 3)): a 4 m wall with a bump, a slanted wall, a floor and
    a far wall with 0.4 % noise and 6 % of the pixels without a depth (as camfeat_cases.depth_image);
    the colour image is random rectangles plus noise."""
    fx, fy, cx, cy = K
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dx, dy = (u - cx) / fx, (v - cy) / fy
    z = np.full((H, W), 4.0)
    z -= 0.6 * np.exp(-((u - 0.23 * W) ** 2 + (v - 0.26 * H) ** 2) / (2.0 * (0.0625 * W) ** 2))
    mid = (u >= 0.38 * W) & (u < 0.69 * W)
    z[mid] = 3.0 / (1.0 - 0.8 * dx[mid])
    floor = (u >= 0.69 * W) & (v > 0.61 * H)
    z[floor] = 1.2 / dy[floor]
    z[v >= 0.8 * H] = 30.0
    z *= 1.0 + 0.004 * rng.standard_normal((H, W))
    d = z.astype(np.float32)
    bad = rng.uniform(size=(H, W)) < 0.06
    d[bad] = rng.choice(np.array([0.0, np.nan, np.inf, -1.0], np.float32), size=int(bad.sum()))
    return d, _blocks(W, H)
