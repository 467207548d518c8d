"""TEST INFRASTRUCTURE — the seeded inputs of the depth pose evidence tests, built on the CPU alone from
the camera view's scenes (camrender_cases.py). tests/test_depth_evidence.py asserts on the restatement
that each case reaches its branch; tests/test_gpu_depth_evidence.py runs the device on them.

If a seeded case breaks a condition of tests/test_depth_evidence.py, change its seed, not the margin."""

import functools

import numpy as np

import camrender_cases as CC
import camrender_restatement as CS
import depthev_restatement as DS

K0 = CC.K0

# the main scene: extrinsics, and the body placed so that the camera sits at the identity
AXIS_BC = np.array([0.1, 1.0, 0.2]) / np.linalg.norm([0.1, 1.0, 0.2])
R_BC = CC._rot((0.1, 1.0, 0.2), 0.1)
T_BC = np.array([0.05, -0.02, 0.1])
POSE_ID = np.concatenate([-R_BC.T @ T_BC, -0.1 * AXIS_BC])   # T_wb = inv(T_bc) as [t, rotvec]
D_STAR = 0.1 * np.array([0.02, -0.015, 0.03, 0.004, -0.006, 0.003])


def base_scene():
    return CC._subset(CC.scene(2), slice(0, 120))


def capped_stack_scene():
    """camrender_cases.stack_scene (every covered pixel stops at t_stop) and one narrow splat of mass
    m_max = 10 in front of it whose mean projects onto the centre of pixel (row 10, column 40): there
    alpha exp(-q / 2) = 1 > alpha_max."""
    b = CC.stack_scene()
    z = 2.5
    mu = np.array([(40.5 - K0[2]) / K0[0] * z, (10.5 - K0[3]) / K0[1] * z, z])
    extra = dict(mu_world=mu[None], Sigma_world=(np.eye(3) * 0.05 ** 2)[None], eta=b["eta"][:1] * 0.5, mass=np.array([10.0]),
                 color=np.array([[0.3, 0.6, 0.9]]))
    return {k: np.concatenate([b[k], extra[k]]) for k in b}


def _render_depth(batch, K, pose6, H, W, cfg, R_bc, t_bc):
    T_cw = CS.camera_from_world(DS.pose_matrix(pose6), R_bc, t_bc)
    return CS.render(batch, [K], [T_cw], H, W, cfg)[0]["depth"][0]


def _noisy(seed, scale=0.02, fill=3.0):
    """The render at the first pose plus seeded noise; `fill` where nothing is rendered."""
    def make(c):
        d = _render_depth(c["batch"], c["K"], c["poses6"][0], c["H"], c["W"], c["cfg"], c["R_bc"], c["t_bc"])
        rng = np.random.default_rng(seed)
        return np.where(d > 0, d + rng.normal(size=d.shape) * scale, fill).astype(np.float32)
    return make


def _moved(c):
    """The render at the first pose moved by D_STAR."""
    T = DS.perturbed(DS.pose_matrix(c["poses6"][0]), D_STAR)
    T_cw = CS.camera_from_world(T, c["R_bc"], c["t_bc"])
    return CS.render(c["batch"], [c["K"]], [T_cw], c["H"], c["W"], c["cfg"])[0]["depth"][0].astype(np.float32)


def _holes(c):
    """_moved with a NaN, an infinity, a zero, a negative and a depth beyond max_depth_m."""
    d = _moved(c).copy()
    d[3, 4], d[10, 12], d[11, 12], d[20, 7], d[25, 25] = np.nan, np.inf, 0.0, -1.0, 60.0
    d[5, 16:20] = np.nan
    return d


def _all_nan(c):
    return np.full((c["H"], c["W"]), np.nan, np.float32)


ZERO6 = np.zeros(6)
_EXT = dict(R_bc=R_BC, t_bc=T_BC)
# name -> (batch builder, poses6 list, extrinsics, H, W, view overrides, evidence overrides, depth builder)
CASES = {
    "extrinsics": (base_scene, [POSE_ID], _EXT, 32, 32, dict(shade=False), dict(max_depth_m=50.0, robust_nu=4.0), _moved),
    "three_poses": (base_scene, [POSE_ID, POSE_ID + 0.3 * D_STAR[::-1], POSE_ID - 2.0 * D_STAR], _EXT, 32, 32,
                    dict(shade=False), dict(max_depth_m=50.0, depth_model="quadratic", depth_sigma_slope=0.002), _moved),
    "cap16": (lambda: CC.scene(1), [ZERO6], {}, CC.H, CC.W, dict(max_splats_per_tile=16), dict(max_depth_m=50.0),
              _noisy(11)),
    "ts8": (lambda: CC._subset(CC.scene(3), slice(0, 100)), [np.array([0.01, -0.02, 0.03, 0.002, 0.001, -0.003])], {}, 32,
            32, dict(tile_size=8), dict(max_depth_m=50.0, robust_nu=4.0), _noisy(12)),
    "stack": (capped_stack_scene, [ZERO6], {}, CC.H, CC.W, dict(), dict(), _noisy(13, 0.01)),
    "invalid": (CC.invalid_scene, [ZERO6], {}, CC.H, CC.W, dict(), dict(max_depth_m=50.0, depth_model="quadratic"),
                _noisy(14)),
    "holes": (base_scene, [POSE_ID], _EXT, 32, 32, dict(shade=False), dict(max_depth_m=50.0, robust_nu=4.0), _holes),
    "all_invalid": (base_scene, [POSE_ID], _EXT, 32, 32, dict(shade=False), dict(), _all_nan),
    "empty": (lambda: CC._subset(CC.scene(1), slice(0, 0)), [ZERO6], {}, 32, 32, dict(), dict(), _noisy(15)),
}


@functools.lru_cache(maxsize=None)
def build(name):
    make, poses, ext, h, w, over, eover, depth = CASES[name]
    c = dict(batch=make(), K=tuple(K0), poses6=np.array(poses, np.float64), R_bc=ext.get("R_bc"), t_bc=ext.get("t_bc"), H=h,
             W=w, cfg=CS.config(**over), ecfg=DS.econfig(**eover))
    c["depth_obs"] = depth(c)
    c["depth_obs"].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement's outputs and conditions for a case, computed once and shared (read-only)."""
    c = build(name)
    out, conds = DS.evidence(c["batch"], c["K"], [DS.pose_matrix(p) for p in c["poses6"]], c["depth_obs"], c["H"], c["W"],
                             c["cfg"], c["ecfg"], c["R_bc"], c["t_bc"])
    for v in out.values():
        v.setflags(write=False)
    return out, conds
