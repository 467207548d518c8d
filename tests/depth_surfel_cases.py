"""Seeded inputs of the depth-surfel tests (test_depth_surfels.py, test_gpu_depth_surfels.py) and the
preconditions they assert on the restatement alone (depth_surfel_restatement.py) before any comparison.

The scene is ray-cast: an oblique camera (pitched down, yawed) over a floor z = 0 and a slightly tilted wall
near x = 3 in the base frame, 2 mm seeded noise on the depth, float32. `planes` adds a foreground sheet
(the depth halved) over the middle eight pixel columns of the second cell column, so depth steps run through
that column of cells, and a NaN, a zero and a beyond-max_depth patch of 12 x 16 pixels in three cells; its rgb
is seeded noise. `grazing` looks along a plane through a long lens, every ray at under 0.1 to the surface.

Preconditions (check_conditions), per case:
 1. the expected numbers of valid cells and of cells each gate rejects first (fill, then plane, then
    incidence), and of kept rows;
 2. at least 0.9 of the valid cells are orientation-determined by surfel_cases.py's criteria
    ((λ1 - λ0)/λ2 >= 1e-4, |n_z| >= 1e-6, ||n_z| - 0.9| >= 1e-6); the normal-dependent fields are
    compared only on such cells;
 3. no gate decision sits within 1e-6 of its threshold: the plane gate relative to (plane_gate σ_z)², on the
    cells that pass the fill gate; the incidence gate absolutely (which is the stricter reading, the
    threshold being below 1), on the cells that pass the other two. The fill gate compares integers."""

import functools

import numpy as np

import depth_surfel_restatement as DR

GATE_MARGIN = 1e-6
DETERMINED_MIN_FRAC = 0.9
NAMES = ("planes", "edge", "overflow", "grazing", "empty", "no_rgb", "quadratic")

_R0 = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])  # camera (x right, y down, z ahead) in the body


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {"y": np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]),
            "z": np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])}[axis]


R_BC = _rot("z", 0.3) @ _rot("y", 0.45) @ _R0  # yawed left, pitched down
T_BC = np.array([0.1, -0.05, 1.2])
_WALL_N = np.array([1.0, 0.15, 0.05]) / np.linalg.norm([1.0, 0.15, 0.05])
_PLANES = ((np.array([0.0, 0.0, 1.0]), 0.0), (_WALL_N, 3.0 * _WALL_N[0]))  # (normal, offset): n . p = offset


def raycast(H, W, K, R, t, planes, seed, noise=0.002):
    """The depth (z of the camera frame) of the nearest plane ahead of every pixel centre, NaN for none."""
    fx, fy, cx, cy = K
    i, j = np.mgrid[0:H, 0:W]
    d = np.stack([(j + 0.5 - cx) / fx, (i + 0.5 - cy) / fy, np.ones((H, W))], axis=-1) @ np.asarray(R).T
    z = np.full((H, W), np.inf)
    for nrm, off in planes:
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (off - nrm @ np.asarray(t)) / (d @ nrm)
        z = np.where((s > 0.0) & (s < z), s, z)
    z = z + np.random.default_rng(seed).normal(scale=noise, size=(H, W))
    return np.where(np.isfinite(z), z, np.nan).astype(np.float32)


def _scene(H, W, seed):
    K = (0.9 * W, 0.9 * W, 0.5 * W, 0.5 * H)
    depth = raycast(H, W, K, R_BC, T_BC, _PLANES, seed)
    rgb = np.random.default_rng(seed + 100).integers(0, 256, (H, W, 3), dtype=np.uint8)
    return depth, rgb, K


@functools.lru_cache(maxsize=None)
def build(name):
    """dict(depth, rgb, K, R, t, timestamp, cfg, base, expect): cfg holds DepthSurfelConfig fields, base the
    base batch's (n_camera_valid) or None, expect the preconditions' numbers."""
    if name in ("planes", "no_rgb", "quadratic"):
        depth, rgb, K = _scene(48, 64, 1)
        depth[:, 20:28] *= np.float32(0.5)     # a foreground sheet: two steps inside the cells of column 1
        depth[0:12, 0:16] = np.nan             # cell 0
        depth[0:12, 48:64] = 0.0               # cell 3
        depth[32:44, 48:64] = 100.0            # cell 11
        cfg = dict(n_feat=16, n_surfel=8)
        if name == "quadratic":
            cfg["depth_model"] = "quadratic"
        # the plane gate rejects column 1 (cells 1, 5, 9) under either depth model, and under the linear one (the
        # smaller sigma) also cell 7, which straddles the crease between the floor and the wall
        n_plane = 3 if name == "quadratic" else 4
        return dict(depth=depth, rgb=None if name == "no_rgb" else rgb, K=K, R=R_BC, t=T_BC, timestamp=12.5, cfg=cfg,
                    base=None, expect=dict(valid=9 - n_plane, fill=3, plane=n_plane, incidence=0, kept=9 - n_plane),
                    plane_rejects=(1, 5, 9), fill_rejects=(0, 3, 11))
    if name == "edge":
        depth, rgb, K = _scene(37, 50, 2)
        return dict(depth=depth, rgb=rgb, K=K, R=R_BC, t=T_BC, timestamp=3.25, cfg=dict(n_feat=16, n_surfel=8, min_fill=0.25),
                    base=None, expect=dict(valid=9, fill=3, plane=0, incidence=0, kept=9))
    if name == "overflow":
        depth, rgb, K = _scene(64, 96, 3)
        return dict(depth=depth, rgb=rgb, K=K, R=R_BC, t=T_BC, timestamp=0.75, cfg=dict(n_feat=16, n_surfel=8, cell_px=8),
                    base=3, expect=dict(valid=None, fill=0, plane=None, incidence=0, kept=13))
    if name == "grazing":
        H, W = 48, 64
        K = (800.0, 800.0, 32.0, 24.0)
        nrm = np.array([1.0, 0.0, -0.05]) / np.linalg.norm([1.0, 0.0, -0.05])  # x_c = 0.05 z_c - 0.1 in the camera frame
        plane = ((R_BC @ nrm, float(nrm @ np.array([-0.1, 0.0, 0.0]) + (R_BC @ nrm) @ T_BC)),)
        depth = raycast(H, W, K, R_BC, T_BC, plane, 4)
        rgb = np.random.default_rng(104).integers(0, 256, (H, W, 3), dtype=np.uint8)
        return dict(depth=depth, rgb=rgb, K=K, R=R_BC, t=T_BC, timestamp=1.0, cfg=dict(n_feat=16, n_surfel=8), base=None,
                    expect=dict(valid=0, fill=0, plane=0, incidence=12, kept=0))
    if name == "empty":
        depth = np.full((48, 64), np.nan, np.float32)
        depth[::2] = 0.0
        depth[::3, ::5] = np.inf
        rgb = np.random.default_rng(105).integers(0, 256, (48, 64, 3), dtype=np.uint8)
        return dict(depth=depth, rgb=rgb, K=(57.6, 57.6, 32.0, 24.0), R=R_BC, t=T_BC, timestamp=1.0,
                    cfg=dict(n_feat=16, n_surfel=8), base=None, expect=dict(valid=0, fill=12, plane=0, incidence=0, kept=0))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def base_arrays(n_feat, n_surfel, n_camera_valid, seed=7):
    """A base batch as a dict: every row of the nine arrays seeded non-zero, the LiDAR slice included."""
    rng = np.random.default_rng(seed)
    n_total = n_feat + n_surfel
    shapes = dict(Lambdas=(3, 3), thetas=(3,), etas=(DR.N_LOBES, 3), weights=(), sources=(), source_indices=(),
                  valid_mask=(), timestamps=(), colors=(3,))
    out = {}
    for k, shp in shapes.items():
        a = rng.uniform(0.1, 5.0, (n_total,) + shp)
        out[k] = a.astype(np.int32) if k in ("sources", "source_indices") else (a > 2.5) if k == "valid_mask" else a
    out.update(n_camera_valid=n_camera_valid, n_lidar_valid=2)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement of a case, computed once and shared; treat it as read-only."""
    c = build(name)
    cfg = dict(DR.DEFAULTS, **c["cfg"])
    base = None if c["base"] is None else base_arrays(cfg["n_feat"], cfg["n_surfel"], c["base"])
    ref = DR.extract(c["depth"], c["rgb"], c["K"], c["R"], c["t"], c["timestamp"], c["cfg"], base)
    ref["case"] = name
    return ref


def stats(ref):
    fill, plane, inc, v = ref["cell_fill_ok"], ref["cell_plane_ok"], ref["cell_inc_ok"], ref["cell_valid"]
    gated = fill & plane
    return dict(n_cells=int(ref["n_cells"]), valid=int(v.sum()), fill=int((~fill).sum()), plane=int((fill & ~plane).sum()),
                incidence=int((gated & ~inc).sum()), kept=int(ref["n_new"]),
                determined=int((v & ref["cell_determined"]).sum()),
                plane_margin=float(ref["plane_margin"][fill].min()) if fill.any() else float("inf"),
                inc_margin=float(ref["inc_margin"][gated].min()) if gated.any() else float("inf"))


def check_conditions(ref):
    """ref: reference(name), which carries its case's name."""
    name = ref["case"]
    s, want = stats(ref), build(name)["expect"]
    for k, v in want.items():
        assert v is None or s[k] == v, (name, k, s)
    for c in build(name).get("plane_rejects", ()):
        assert ref["cell_fill_ok"][c] and not ref["cell_plane_ok"][c], (name, c)
    for c in build(name).get("fill_rejects", ()):
        assert not ref["cell_fill_ok"][c], (name, c)
    if name == "overflow":
        assert s["valid"] > ref["free"] == 13 and ref["n_in"] == 3, (name, s)
    assert s["valid"] +s["fill"] + s["plane"] + s["incidence"] == s["n_cells"], (name, s)
    assert s["determined"] >= DETERMINED_MIN_FRAC * s["valid"], (name, s)
    assert s["plane_margin"] >= GATE_MARGIN and s["inc_margin"] >= GATE_MARGIN, (name, s)
    return s
