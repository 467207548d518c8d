"""TEST INFRASTRUCTURE — the seeded inputs of the photometric pose evidence tests, built on the CPU alone from
the camera view's and the depth evidence's scenes (camrender_cases.py, depthev_cases.py), all 32 x 32 or
48 x 64: the smallest frames that reach each branch. tests/test_photo_evidence.py asserts on the restatement
that each case reaches its branch; tests/test_gpu_photo_evidence.py runs the device on them.

If a seeded case breaks a condition of tests/test_photo_evidence.py, change its seed, not the margin."""

import functools

import numpy as np

import camrender_cases as CC
import camrender_restatement as CS
import depthev_cases as DC
import depthev_restatement as DS
import photoev_restatement as PS

K0, POSE_ID, D_STAR, ZERO6, _EXT = DC.K0, DC.POSE_ID, DC.D_STAR, DC.ZERO6, DC._EXT


def render_luminance(batch, K, pose6_or_T, H, W, cfg, R_bc, t_bc, weights):
    """Y / A of camrender_restatement.render at a pose ([t, rotvec] or T_wb) with a zero background: w . images
    over alpha where alpha > eps, 0 elsewhere; and alpha."""
    T_wb = np.asarray(pose6_or_T, np.float64)
    T_wb = T_wb if T_wb.shape == (4, 4) else DS.pose_matrix(T_wb)
    out = CS.render(batch, [K], [CS.camera_from_world(T_wb, R_bc, t_bc)], H, W, dict(cfg, background=(0.0, 0.0, 0.0)))[0]
    A = out["alpha"][0]
    Y = PS.luminance(out["images"][0], weights)
    return np.where(A > cfg["eps"], Y / np.where(A > cfg["eps"], A, 1.0), 0.0), A


def _at(c, pose6_or_T):
    return render_luminance(c["batch"], c["K"], pose6_or_T, c["H"], c["W"], c["cfg"], c["R_bc"], c["t_bc"],
                            c["pcfg"]["weights"])[0]


def _moved(c):
    """The luminance rendered at the first pose moved by D_STAR."""
    return _at(c, DS.perturbed(DS.pose_matrix(c["poses6"][0]), D_STAR)).astype(np.float32)


def _noisy(seed, scale=0.03):
    """The luminance rendered at the first pose plus seeded noise."""
    def make(c):
        rng = np.random.default_rng(seed)
        y = _at(c, c["poses6"][0])
        return (y + rng.normal(size=y.shape) * scale).astype(np.float32)
    return make


def _holes(c):
    """_moved with NaNs, an infinity and a negative infinity."""
    y = _moved(c).copy()
    y[3, 4], y[10, 12], y[11, 12] = np.nan, np.inf, -np.inf
    y[5, 16:20] = np.nan
    return y


def _all_nan(c):
    return np.full((c["H"], c["W"]), np.nan, np.float32)


def _rgb8(c):
    """The colour over the coverage rendered at the first pose moved by D_STAR (black where nothing is
    rendered), as an 8-bit camera would give it."""
    T = DS.perturbed(DS.pose_matrix(c["poses6"][0]), D_STAR)
    out = CS.render(c["batch"], [c["K"]], [CS.camera_from_world(T, c["R_bc"], c["t_bc"])], c["H"], c["W"], c["cfg"])[0]
    A = out["alpha"][0][..., None]
    rgb = np.where(A > c["cfg"]["eps"], out["images"][0] / np.where(A > c["cfg"]["eps"], A, 1.0), 0.0)
    return np.clip(np.rint(rgb * 255.0), 0, 255).astype(np.uint8)


_BASE = (DC.base_scene, [POSE_ID], _EXT, 32, 32)
# name -> (batch builder, poses6 list, extrinsics, H, W, view overrides, evidence overrides, observation builder)
CASES = {
    "shaded": _BASE + (dict(shade=True), dict(robust_nu=4.0), _moved),
    "unshaded": _BASE + (dict(shade=False), dict(), _moved),
    "three_poses": (DC.base_scene, [POSE_ID, POSE_ID + 0.3 * D_STAR[::-1], POSE_ID - 2.0 * D_STAR], _EXT, 32, 32, dict(),
                    dict(sigma=0.08), _moved),
    "cap16": (lambda: CC.scene(1), [ZERO6], {}, CC.H, CC.W, dict(max_splats_per_tile=16), dict(), _noisy(21)),
    "ts8": (lambda: CC._subset(CC.scene(3), slice(0, 100)), [np.array([0.01, -0.02, 0.03, 0.002, 0.001, -0.003])], {}, 32,
            32, dict(tile_size=8), dict(robust_nu=4.0), _noisy(22)),
    "stack": (DC.capped_stack_scene, [ZERO6], {}, CC.H, CC.W, dict(), dict(), _noisy(23, 0.01)),
    "invalid": (CC.invalid_scene, [ZERO6], {}, CC.H, CC.W, dict(), dict(robust_nu=2.5), _noisy(24)),
    "background": _BASE + (dict(shade=True, background=(0.25, 0.5, 0.75)), dict(robust_nu=4.0), _moved),
    "rgb8": _BASE + (dict(shade=True), dict(robust_nu=4.0), _rgb8),
    "holes": _BASE + (dict(shade=True), dict(robust_nu=4.0), _holes),
    "all_nan": _BASE + (dict(shade=True), dict(), _all_nan),
    "empty": (lambda: CC._subset(CC.scene(1), slice(0, 0)), [ZERO6], {}, 32, 32, dict(), dict(), _noisy(25)),
    "weights": _BASE + (dict(shade=True), dict(weights=(0.5, -0.25, 1.0)), _moved),
}


@functools.lru_cache(maxsize=None)
def build(name):
    """image_obs is what the operator is given ((H, W, 3) uint8 or (H, W) float32), lum_obs the float32
    luminance it observes; ecfg is the depth evidence's configuration in the joint tests (depth_obs below)."""
    make, poses, ext, h, w, over, pover, obs = CASES[name]
    c = dict(batch=make(), K=tuple(K0), poses6=np.array(poses, np.float64), R_bc=ext.get("R_bc"), t_bc=ext.get("t_bc"), H=h,
             W=w, cfg=CS.config(**over), pcfg=PS.pconfig(**pover), ecfg=DS.econfig(max_depth_m=50.0, robust_nu=4.0))
    c["image_obs"] = obs(c)
    c["lum_obs"] = PS.image_luminance(c["image_obs"], c["pcfg"]["weights"]) if c["image_obs"].ndim == 3 else c["image_obs"]
    for k in ("image_obs", "lum_obs"):
        c[k].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def depth_obs(name):
    """The depth frame beside the case's image in the joint tests: depthev_cases' render at the moved pose."""
    d = DC._moved(build(name))
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement's outputs and conditions for a case, computed once and shared (read-only)."""
    c = build(name)
    out, conds = PS.evidence(c["batch"], c["K"], [DS.pose_matrix(p) for p in c["poses6"]], c["lum_obs"], c["H"], c["W"],
                             c["cfg"], c["pcfg"], c["R_bc"], c["t_bc"])
    for v in out.values():
        v.setflags(write=False)
    return out, conds


@functools.lru_cache(maxsize=None)
def restated_depth(name):
    """depthev_restatement's outputs for the case's depth_obs and ecfg: the depth row of the joint evidence."""
    c = build(name)
    out, _ = DS.evidence(c["batch"], c["K"], [DS.pose_matrix(p) for p in c["poses6"]], depth_obs(name), c["H"], c["W"],
                         c["cfg"], c["ecfg"], c["R_bc"], c["t_bc"])
    for v in out.values():
        v.setflags(write=False)
    return out
