"""The depth pose evidence on the CPU: the restatement (tests/depthev_restatement.py) held to central
differences of the camera view's restatement and to closed forms, the seeded cases (tests/depthev_cases.py)
held to the branches they are there for, and the wrapper's argument errors, which need no device."""

import numpy as np
import pytest

import camrender_cases as CC
import camrender_restatement as CS
import depthev_cases as DC
import depthev_restatement as DS
from gcslam import _header
from gcslam.ops import DepthEvidenceConfig, PinholeIntrinsics, depth_pose_evidence_batched
from gcslam.rendering import CameraViewConfig


def test_header_declares_the_entries():
    protos, structs, consts = _header.load()
    assert "gc_camera_splat_jvp" in protos and "gc_depth_pose_evidence" in protos
    assert consts["GC_DEPTHEV_PARTS"] == 46 == DS.PARTS and consts["GC_DEPTHEV_PARTIAL"] == 31


def _render_at(c, T_wb):
    T_cw = CS.camera_from_world(T_wb, c["R_bc"], c["t_bc"])
    return CS.render(c["batch"], [c["K"]], [T_cw], c["H"], c["W"], c["cfg"])[0]


def test_jacobian_against_central_differences():
    """The restatement's J against central differences of camrender_restatement.render at step 1e-6, where
    the +-step renders keep valid, the lists and n_contrib: 1e-6 of max |J| per axis."""
    c = DC.build("extrinsics")
    out, conds = DC.restated("extrinsics")
    assert conds[0]["clamped"] > 0  # the tangent clamp is differentiated too
    T0 = DS.pose_matrix(c["poses6"][0])
    base = _render_at(c, T0)
    assert np.array_equal(base["depth"][0], out["depth"][0])
    covered = base["alpha"][0] > c["cfg"]["eps"]
    step = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = step
        hi, lo = _render_at(c, DS.perturbed(T0, d)), _render_at(c, DS.perturbed(T0, -d))
        for side in (hi, lo):
            for key in ("valid", "tile_indices", "tile_counts", "n_contrib"):
                assert np.array_equal(side[key], base[key]), (k, key)
        fd = (hi["depth"][0] - lo["depth"][0]) / (2.0 * step)
        J = out["J"][0, :, :, k]
        scale = np.max(np.abs(J[covered]))
        err = np.max(np.abs(fd[covered] - J[covered])) / scale
        print(f"axis {k}: max |J| = {scale:.4g}, |J - fd| / max |J| = {err:.3g}")
        assert err < 1e-6, (k, err)


def test_one_splat_translation_along_the_axis():
    """One isotropic splat on the optical axis: the rendered depth is its z wherever it covers, so moving
    the body along z gives J_z = -1 there and the lateral translations give 0."""
    batch = dict(mu_world=np.array([[0.0, 0.0, 4.0]]), Sigma_world=(np.eye(3) * 0.3 ** 2)[None],
                 eta=np.zeros((1, 1, 3)), mass=np.ones(1), color=np.ones((1, 3)))
    K = (20.0, 20.0, 8.0, 8.0)
    cfg = CS.config(shade=False)
    e = DS.evidence_one(batch, K, np.eye(4), np.full((16, 16), 4.0, np.float32), 16, 16, cfg, DS.econfig())
    covered = e["render"]["alpha"] > cfg["eps"]
    assert covered.sum() > 20
    assert np.max(np.abs(e["J"][covered][:, 2] + 1.0)) < 1e-12
    assert np.max(np.abs(e["J"][covered][:, :2])) < 1e-12


@pytest.mark.parametrize("name", ["extrinsics", "cap16", "stack"])
def test_no_evidence_from_the_render_itself(name):
    c = DC.build(name)
    out, _ = DC.restated(name)
    e = DS.evidence_one(c["batch"], c["K"], DS.pose_matrix(c["poses6"][0]), out["depth"][0], c["H"], c["W"], c["cfg"],
                        c["ecfg"], c["R_bc"], c["t_bc"])
    assert e["n_used"] > 0 and e["cost"] == 0.0 and not e["h6"].any() and e["L6"].any()


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_L_is_symmetric_and_psd(name):
    out, _ = DC.restated(name)
    for L in out["L6"]:
        assert np.array_equal(L, L.T) or np.max(np.abs(L - L.T)) <= 1e-15 * np.max(np.abs(L))
        if L.any():
            assert np.linalg.eigvalsh(0.5 * (L + L.T)).min() >= -1e-12 * np.linalg.norm(L)
    assert np.array_equal(out["L_pose"][:, 6:], np.zeros_like(out["L_pose"][:, 6:]))
    assert np.array_equal(out["L_pose"][:, :, 6:], np.zeros_like(out["L_pose"][:, :, 6:]))


@pytest.mark.parametrize("nu", [4.0, None])
def test_one_gauss_newton_step_recovers_the_motion(nu):
    """depth_obs rendered at the pose moved by d*: one step (L6 + 1e-9 I)^-1 h6 from the unmoved pose
    recovers d* to 10 %."""
    c = DC.build("extrinsics")
    ecfg = DS.econfig(min_depth_m=0.1, max_depth_m=50.0, robust_nu=nu)
    if nu == c["ecfg"]["robust_nu"] and ecfg == c["ecfg"]:
        e = {k: v[0] for k, v in DC.restated("extrinsics")[0].items()}
    else:
        e = DS.evidence_one(c["batch"], c["K"], DS.pose_matrix(c["poses6"][0]), c["depth_obs"], c["H"], c["W"], c["cfg"],
                            ecfg, c["R_bc"], c["t_bc"])
    step = np.linalg.solve(e["L6"] + 1e-9 * np.eye(6), e["h6"])
    rel = np.linalg.norm(step - DC.D_STAR) / np.linalg.norm(DC.D_STAR)
    print(f"nu = {nu}: n_used = {int(e['n_used'])}, |step - d*| / |d*| = {rel:.4f}")
    assert rel < 0.1


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_cases_pin_an_implementation(name):
    """The margins of tests/test_camera_render.py at every pose of every case, and no observed depth at a
    limit: an implementation that rounds differently takes the same branches."""
    c = DC.build(name)
    out, conds = DC.restated(name)
    for cd in conds:
        assert cd["bbox_margin"] >= 1e-9 and cd["depth_gap"] >= 1e-9
        assert cd["skip_margin"] >= 1e-9 and cd["stop_margin"] >= 1e-9 and cd["z_margin"] >= 1e-9
    obs = c["depth_obs"][np.isfinite(c["depth_obs"])].astype(np.float64)
    for lim in (c["ecfg"]["min_depth_m"], c["ecfg"]["max_depth_m"]):
        assert obs.size == 0 or np.min(np.abs(obs - lim)) > 1e-6
    alpha = out["alpha"]
    assert not ((alpha > 0) & (np.abs(alpha - c["cfg"]["eps"]) < 1e-13)).any()


def test_each_case_reaches_its_branch():
    out, conds = DC.restated("extrinsics")
    assert conds[0]["clamped"] > 0 and conds[0]["skipped"] > 0 and out["n_used"][0] > 500
    out3, conds3 = DC.restated("three_poses")
    assert out3["L6"].shape == (3, 6, 6) and not np.array_equal(out3["L6"][0], out3["L6"][1])
    assert np.array_equal(out3["J"][0], out["J"][0])  # the same first pose: J does not read the evidence's settings
    _, cc = DC.restated("cap16")
    assert cc[0]["cut"] > 0
    outs, cs = DC.restated("stack")
    assert cs[0]["stopped"] > 0 and cs[0]["alpha_capped"] > 0
    outi, _ = DC.restated("invalid")
    for r in CC.INVALID_ROWS:
        assert not outi["dmeans_px"][0, r].any() and not outi["ddepths"][0, r].any() and not outi["dSigmas_inv"][0, r].any()
    assert outi["ddepths"][0, 0].any()
    outh, _ = DC.restated("holes")
    ch = DC.build("holes")
    holes = ~np.isfinite(ch["depth_obs"]) | (ch["depth_obs"] <= 0.05) | (ch["depth_obs"] >= 50.0)
    assert holes.sum() >= 8 and not outh["used"][0][holes].any()
    assert not outh["residual"][0][holes].any() and not outh["weight"][0][holes].any()
    assert outh["n_used"][0] == out["n_used"][0] - int((holes & out["used"][0]).sum()) < out["n_used"][0]
    for name in ("all_invalid", "empty"):
        o, _ = DC.restated(name)
        assert o["n_used"][0] == 0 and not o["L6"].any() and not o["h_pose"].any() and not o["parts"].any()
        assert np.array_equal(o["L_pose"][0, :6, :6], 1e-9 * np.eye(6))
    o8, c8 = DC.restated("ts8")
    assert DC.build("ts8")["cfg"]["tile_size"] == 8 and o8["n_used"][0] > 0


K_OK = PinholeIntrinsics(fx=60.0, fy=60.0, cx=16.0, cy=16.0)
D_OK = np.ones((32, 32), np.float32)
P_OK = np.zeros((1, 6))


@pytest.mark.parametrize("kw, word", [
    (dict(poses6=np.zeros((33, 6))), "poses"),
    (dict(poses6=np.zeros((0, 6))), "poses"),
    (dict(poses6=np.zeros((2, 5))), "poses6"),
    (dict(poses6=np.array([[0, 0, 0, 0, np.nan, 0.0]])), "finite"),
    (dict(view_cfg=CameraViewConfig(tile_size=32)), "tile_size"),
    (dict(depth_obs=np.ones((32, 32, 1), np.float32)), "depth_obs"),
    (dict(depth_obs=np.ones((30, 32), np.float32)), "multiple of tile_size"),
    (dict(R_base_camera=np.eye(3) * 1.1), "rotation"),
    (dict(R_base_camera=np.eye(4)), "R_base_camera"),
    (dict(t_base_camera=[0.0, np.inf, 0.0]), "finite"),
    (dict(cfg=DepthEvidenceConfig(depth_sigma0=0.0)), "depth_sigma0"),
    (dict(cfg=DepthEvidenceConfig(depth_sigma_slope=-1.0)), "depth_sigma_slope"),
    (dict(cfg=DepthEvidenceConfig(robust_nu=0.0)), "robust_nu"),
    (dict(cfg=DepthEvidenceConfig(min_depth_m=5.0, max_depth_m=5.0)), "depth limits"),
    (dict(cfg=DepthEvidenceConfig(depth_model="cubic")), "depth_model"),
    (dict(cfg=DepthEvidenceConfig(max_depth_m=np.nan)), "finite"),
    (dict(intrinsics=(60.0, 60.0, 16.0, 16.0)), "PinholeIntrinsics"),
    (dict(accumulate_into=(np.zeros((1, 22, 22)), np.zeros((1, 22)))), "accumulate_into"),
])
def test_wrapper_refuses_before_a_device(kw, word):
    """The batch argument is checked last, so an object that is no batch shows that no device was asked for."""
    args = dict(intrinsics=K_OK, poses6=P_OK, depth_obs=D_OK)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        depth_pose_evidence_batched(object(), **args)
    with pytest.raises(ValueError, match="cannot render"):
        depth_pose_evidence_batched(object(), K_OK, P_OK, D_OK)
