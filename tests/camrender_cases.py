"""TEST INFRASTRUCTURE — the seeded inputs of the camera view tests, built on the CPU alone (the pattern
of render_cases.py). tests/test_camera_render.py asserts on the restatement the conditions under which
they pin an implementation and that each case reaches its branch; tests/test_gpu_camera_render.py runs
the device on them.

If a seeded case breaks a condition of tests/test_camera_render.py, change its seed, not the margin."""

import functools

import numpy as np

import camrender_restatement as CS

L = 3
H, W = 48, 64
K0 = (60.0, 60.0, 32.0, 24.0)   # fx, fy, cx, cy


def _sigma3(rng, n, lo, hi):
    """n covariances with standard deviations in [lo, hi] along random axes."""
    Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    ev = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 3))) ** 2
    S = np.einsum("nij,nj,nkj->nik", Q, ev, Q)
    return 0.5 * (S + np.swapaxes(S, 1, 2))


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)


def pose(axis, angle, t):
    """T_cw from a rotation (axis, angle) and a translation."""
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = _rot(axis, angle), t
    return T


def scene(seed, n=300):
    """n primitives with sigma 0.03-0.25 m at 2-12 m in front of an identity camera, over the 48 x 64
    frame of K0 and a little beyond its clamp at 1.3 x the half extent (so some sit at the tangent clamp), and one exact depth tie:
    primitives 10 and 200 share z."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(2.0, 12.0, n)
    mu = np.column_stack([rng.uniform(-0.73, 0.73, n) * z, rng.uniform(-0.55, 0.55, n) * z, z])
    mu[200, 2] = mu[10, 2]
    mu[200, :2] = mu[10, :2] + [0.05, -0.04]
    eta = rng.normal(size=(n, L, 3)) * 2.0
    eta[::7, 2] = 0.0
    return dict(mu_world=mu, Sigma_world=_sigma3(rng, n, 0.03, 0.25), eta=eta, mass=rng.uniform(0.05, 1.0, n),
                color=rng.uniform(0.0, 1.0, (n, 3)))


def _subset(b, sel):
    return {k: np.ascontiguousarray(v[sel]) for k, v in b.items()}


def stack_scene():
    """Eight co-located broad splats at depths 3.0 .. 3.7, listed back to front by index, mass 8, and one
    off-frame primitive of mass 10: alpha = 0.8 each, so a pixel's T falls below t_stop = 1e-4 after six
    (0.2^6 = 6.4e-5) where the Gaussians are near their peak."""
    n = 9
    mu = np.zeros((n, 3))
    mu[:8, 2] = 3.7 - 0.1 * np.arange(8)
    mu[:8, 0], mu[:8, 1] = 0.01, -0.02
    mu[8] = [40.0, 0.0, 5.0]
    Sig = np.tile(np.eye(3) * 4.0, (n, 1, 1))     # sigma 2 m at 3 m: ~40 px
    Sig[8] = np.eye(3) * 0.01
    rng = np.random.default_rng(5)
    return dict(mu_world=mu, Sigma_world=Sig, eta=rng.normal(size=(n, L, 3)), mass=np.array([8.0] * 8 + [10.0]),
                color=rng.uniform(0.2, 1.0, (n, 3)))


def invalid_scene():
    """The seed-2 scene's first 60 with primitives behind the camera, nearer than near, beyond far, and
    one with a NaN mean and one with an infinite covariance entry."""
    b = _subset(scene(2), slice(0, 60))
    b["mu_world"][3] = [0.1, 0.2, -4.0]
    b["mu_world"][7] = [0.0, 0.0, 0.1]
    b["mu_world"][11] = [1.0, 2.0, 150.0]
    b["mu_world"][13] = [np.nan, 0.0, 5.0]
    b["Sigma_world"][17, 1, 1] = np.inf
    return b


INVALID_ROWS = (3, 7, 11, 13, 17)

# name -> (batch builder, [K per view], [T_cw per view], H, W, config overrides)
_TWO_VIEWS = ([K0, (45.0, 50.0, 30.0, 26.0)],
              [pose((0.2, 1.0, 0.1), 0.15, (0.3, -0.2, 0.5)), pose((1.0, -0.3, 0.2), -0.2, (-0.4, 0.1, 1.0))])
CASES = {
    "cap16": (lambda: scene(1), [K0], [np.eye(4)], H, W, dict(max_splats_per_tile=16)),
    "cap256": (lambda: scene(1), [K0], [np.eye(4)], H, W, dict()),
    "two_views": (lambda: scene(3), _TWO_VIEWS[0], _TWO_VIEWS[1], H, W, dict()),
    "invalid": (invalid_scene, [K0], [np.eye(4)], H, W, dict()),
    "stack": (stack_scene, [K0], [np.eye(4)], H, W, dict()),
    "no_shade": (lambda: _subset(scene(2), slice(0, 120)), [K0], [np.eye(4)], 32, 32, dict(shade=False)),
    "background": (lambda: _subset(scene(2), slice(0, 120)), [K0], [np.eye(4)], 32, 32,
                   dict(background=(0.25, 0.5, 0.75))),
    "one_tile": (lambda: _subset(scene(3), slice(0, 150)), [(20.0, 20.0, 8.0, 8.0)], [np.eye(4)], 16, 16, dict()),
    "cap1": (lambda: _subset(scene(2), slice(0, 120)), [K0], [np.eye(4)], 32, 32, dict(max_splats_per_tile=1)),
    "three_views_ts8": (lambda: _subset(scene(3), slice(0, 100)), [K0, K0, (50.0, 55.0, 15.0, 17.0)],
                        [np.eye(4)] + _TWO_VIEWS[1], 32, 32, dict(tile_size=8)),
    "empty": (lambda: _subset(scene(1), slice(0, 0)), [K0], [np.eye(4)], 32, 32, dict(background=(0.1, 0.2, 0.3))),
}


def build(name):
    make, Ks, Ts, h, w, over = CASES[name]
    return dict(batch=make(), Ks=[tuple(k) for k in Ks], T_cws=[np.asarray(T, np.float64) for T in Ts], H=h, W=w,
                cfg=CS.config(**over))


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement's outputs and conditions for a case, computed once and shared (read-only)."""
    c = build(name)
    out, conds = CS.render(c["batch"], c["Ks"], c["T_cws"], c["H"], c["W"], c["cfg"])
    for v in out.values():
        v.setflags(write=False)
    return out, conds


def err_frac(got, want):
    """max |got - want| over the finite entries of want, as a fraction of their max-abs; the non-finite
    entries must agree exactly."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin])
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - want[fin]))) / max(float(np.max(np.abs(want[fin]))), 1e-300)
