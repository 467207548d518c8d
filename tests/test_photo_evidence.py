"""The photometric pose evidence on the CPU: the restatement (tests/photoev_restatement.py) held to central
differences of the camera view's restatement and to closed forms, the seeded cases (tests/photoev_cases.py)
held to the branches they are there for, and the wrappers' argument errors, which need no device."""

import numpy as np
import pytest

import camrender_cases as CC
import camrender_restatement as CS
import depthev_cases as DC
import depthev_restatement as DS
import photoev_cases as PC
import photoev_restatement as PS
from gcslam import _header
from gcslam.ops import (DepthEvidenceConfig, PhotometricEvidenceConfig, PinholeIntrinsics, luminance_image,
                        photometric_pose_evidence_batched, rgbd_pose_evidence_batched)
from gcslam.ops.photometric_pose_evidence import GREY_WEIGHTS
from gcslam.rendering import CameraViewConfig


def test_header_declares_the_entries():
    protos, structs, consts = _header.load()
    for name in ("gc_camera_shade_jvp", "gc_photo_pose_evidence", "gc_rgbd_pose_evidence", "gc_image_luminance"):
        assert name in protos, name
    assert len(protos["gc_photo_pose_evidence"][0]) == 28 and len(protos["gc_rgbd_pose_evidence"][0]) == 40
    assert consts["GC_DEPTHEV_PARTS"] == PS.PARTS == 46
    assert PS.GREY == GREY_WEIGHTS == PhotometricEvidenceConfig().weights
    assert PhotometricEvidenceConfig().sigma == PS.PCFG["sigma"] == 0.05


# ------------------------------------------------------------------------------------ finite differences
def test_shading_tangent_against_central_differences():
    """The shading tangent of every primitive of the shaded scene (lobes with eta = 0 among them) against
    central differences of camrender_restatement.vmf_shading over the pose, step 1e-6: 1e-6 of max |ds| per
    axis. Zero where the view is not shaded."""
    c = PC.build("shaded")
    T0 = DS.pose_matrix(c["poses6"][0])
    eta, mu = np.asarray(c["batch"]["eta"], np.float64), np.asarray(c["batch"]["mu_world"], np.float64)
    n = mu.shape[0]
    assert (np.abs(eta).sum(axis=2) == 0).any()
    centre = lambda T_wb: (lambda T: -T[:3, :3].T @ T[:3, 3])(CS.camera_from_world(T_wb, c["R_bc"], c["t_bc"]))
    c0, dc = PS.centre_tangents(CS.camera_from_world(T0, c["R_bc"], c["t_bc"]), T0[:3, 3])
    assert np.array_equal(c0, centre(T0))
    ds = np.stack([PS.shading_tangent(c0 - mu[i], dc, eta[i]) for i in range(n)])
    step = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = step
        hi, lo = centre(DS.perturbed(T0, d)), centre(DS.perturbed(T0, -d))
        fd = np.array([(CS.vmf_shading(hi - mu[i], eta[i]) - CS.vmf_shading(lo - mu[i], eta[i])) / (2.0 * step)
                       for i in range(n)])
        scale = np.max(np.abs(ds[:, k]))
        err = np.max(np.abs(fd - ds[:, k])) / scale
        print(f"axis {k}: max |ds| = {scale:.4g}, |ds - fd| / max |ds| = {err:.3g}")
        assert scale > 0 and err < 1e-6, (k, err)
    out, _ = PC.restated("shaded")
    wc = PS.luminance(c["batch"]["color"], PS.GREY)
    assert np.array_equal(out["dlum"][0], wc[:, None] * ds) and out["dlum"].any()
    flat, _ = PC.restated("unshaded")
    assert not flat["dlum"].any() and flat["lum"].any()
    assert np.array_equal(flat["lum"][0], PS.luminance(c["batch"]["color"], PS.GREY))


def test_jacobian_against_central_differences():
    """The restatement's J against central differences of w . images / alpha of camrender_restatement.render
    at step 1e-6 on the shaded scene with extrinsics, where the +-step renders keep valid, the lists and
    n_contrib: 1e-6 of max |J| per axis."""
    c = PC.build("shaded")
    out, conds = PC.restated("shaded")
    assert conds[0]["clamped"] > 0
    T0 = DS.pose_matrix(c["poses6"][0])

    def at(T_wb):
        r = CS.render(c["batch"], [c["K"]], [CS.camera_from_world(T_wb, c["R_bc"], c["t_bc"])], c["H"], c["W"], c["cfg"])[0]
        return r, PS.luminance(r["images"][0], PS.GREY) / np.where(r["alpha"][0] > c["cfg"]["eps"], r["alpha"][0], 1.0)

    base, y0 = at(T0)
    covered = base["alpha"][0] > c["cfg"]["eps"]
    assert np.max(np.abs(y0 - out["lum_render"][0])[covered]) < 1e-14
    step = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = step
        (hi, yh), (lo, yl) = at(DS.perturbed(T0, d)), at(DS.perturbed(T0, -d))
        for side in (hi, lo):
            for key in ("valid", "tile_indices", "tile_counts", "n_contrib"):
                assert np.array_equal(side[key], base[key]), (k, key)
        fd = (yh - yl) / (2.0 * step)
        J = out["J"][0, :, :, k]
        scale = np.max(np.abs(J[covered]))
        err = np.max(np.abs(fd[covered] - J[covered])) / scale
        print(f"axis {k}: max |J| = {scale:.4g}, |J - fd| / max |J| = {err:.3g}")
        assert err < 1e-6, (k, err)


# ------------------------------------------------------------------------------------------ closed forms
def test_one_unshaded_splat_has_no_gradient():
    """One unshaded splat: Y / A is its luminance wherever it covers, whatever the pose."""
    batch = dict(mu_world=np.array([[0.1, -0.05, 4.0]]), Sigma_world=(np.eye(3) * 0.3 ** 2)[None],
                 eta=np.zeros((1, 1, 3)), mass=np.ones(1), color=np.array([[0.2, 0.7, 0.4]]))
    K = (20.0, 20.0, 8.0, 8.0)
    cfg = CS.config(shade=False)
    e = PS.evidence_one(batch, K, np.eye(4), np.full((16, 16), 0.5, np.float32), 16, 16, cfg, PS.pconfig())
    covered = e["render"]["alpha"] > cfg["eps"]
    assert covered.sum() > 20 and e["n_used"] == covered.sum()
    assert np.max(np.abs(e["J"][covered])) < 1e-12
    # A = 1 - (1 - a) carries the rounding of 1 - a, 2^-53 absolute, so 2^-53 / a relative with a >= alpha_skip
    y = PS.luminance(batch["color"][0], PS.GREY)
    assert np.max(np.abs(e["lum_render"][covered] - y)) < y * 2.0 ** -52 / cfg["alpha_skip"]


@pytest.mark.parametrize("name", ["shaded", "cap16", "stack"])
def test_no_evidence_from_the_render_itself(name):
    c = PC.build(name)
    out, _ = PC.restated(name)
    e = PS.evidence_one(c["batch"], c["K"], DS.pose_matrix(c["poses6"][0]), out["lum_render"][0], c["H"], c["W"], c["cfg"],
                        c["pcfg"], c["R_bc"], c["t_bc"])
    assert e["n_used"] > 0 and e["cost"] == 0.0 and not e["h6"].any() and e["L6"].any()


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_L_is_symmetric_and_psd(name):
    out, _ = PC.restated(name)
    for L in out["L6"]:
        assert np.array_equal(L, L.T) or np.max(np.abs(L - L.T)) <= 1e-15 * np.max(np.abs(L))
        if L.any():
            assert np.linalg.eigvalsh(0.5 * (L + L.T)).min() >= -1e-12 * np.linalg.norm(L)
    assert np.array_equal(out["L_pose"][:, 6:], np.zeros_like(out["L_pose"][:, 6:]))
    assert np.array_equal(out["L_pose"][:, :, 6:], np.zeros_like(out["L_pose"][:, :, 6:]))


# --------------------------------------------------------------------------------------- one Gauss-Newton step
def _gn(L6, h6):
    step = np.linalg.solve(L6 + 1e-9 * np.eye(6), h6)
    return np.linalg.norm(step - PC.D_STAR) / np.linalg.norm(PC.D_STAR)


@pytest.mark.parametrize("shade", [True, False])
@pytest.mark.parametrize("nu", [4.0, None])
def test_one_gauss_newton_step_recovers_the_motion(shade, nu):
    """lum_obs rendered at the pose moved by d*, sigma = 0.05: one step (L6 + 1e-9 I)^-1 h6 from the unmoved
    pose recovers d* to 10 %, the depth evidence's bar."""
    name = "shaded" if shade else "unshaded"
    c = PC.build(name)
    pcfg = PS.pconfig(robust_nu=nu)
    assert pcfg["sigma"] == 0.05
    if pcfg == c["pcfg"]:
        e = {k: v[0] for k, v in PC.restated(name)[0].items()}
    else:
        e = PS.evidence_one(c["batch"], c["K"], DS.pose_matrix(c["poses6"][0]), c["lum_obs"], c["H"], c["W"], c["cfg"], pcfg,
                            c["R_bc"], c["t_bc"])
    rel = _gn(e["L6"], e["h6"])
    print(f"shade = {shade}, nu = {nu}: n_used = {int(e['n_used'])}, cost = {float(e['cost']):.3g}, "
          f"cond(L6) = {np.linalg.cond(e['L6']):.3g}, |step - d*| / |d*| = {rel:.4f}")
    assert e["n_used"] == 909 and rel < 0.1


def test_one_joint_gauss_newton_step_recovers_the_motion():
    """The RGB-D evidence, depth plus luminance with their default sigmas, is held to the same 10 %; each part
    alone is under 5 %."""
    d, y = PC.restated_depth("shaded"), PC.restated("shaded")[0]
    parts = dict(depth=_gn(d["L6"][0], d["h6"][0]), luminance=_gn(y["L6"][0], y["h6"][0]),
                 joint=_gn(d["L6"][0] + y["L6"][0], d["h6"][0] + y["h6"][0]))
    print("|step - d*| / |d*|:", {k: float("%.4f" % v) for k, v in parts.items()},
          "trace ratio depth / luminance: %.3g" % (np.trace(d["L6"][0]) / np.trace(y["L6"][0])))
    assert parts["depth"] < 0.05 and parts["luminance"] < 0.05
    assert parts["joint"] < 0.1


# ------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_cases_pin_an_implementation(name):
    """The depth cases' margins at every pose of every case: an implementation that rounds differently takes
    the same branches."""
    c = PC.build(name)
    out, conds = PC.restated(name)
    for cd in conds:
        assert cd["bbox_margin"] >= 1e-9 and cd["depth_gap"] >= 1e-9
        assert cd["skip_margin"] >= 1e-9 and cd["stop_margin"] >= 1e-9 and cd["z_margin"] >= 1e-9
    alpha = out["alpha"]
    assert not ((alpha > 0) & (np.abs(alpha - c["cfg"]["eps"]) < 1e-13)).any()


def test_each_case_reaches_its_branch():
    out, conds = PC.restated("shaded")
    assert conds[0]["clamped"] > 0 and conds[0]["skipped"] > 0 and out["n_used"][0] > 500
    c = PC.build("shaded")
    eta0 = np.abs(np.asarray(c["batch"]["eta"])).sum(axis=2) == 0
    assert eta0.any() and out["valid"][0][eta0.any(axis=1)].any()   # a lobe with eta = 0 on a rendered primitive
    flat, _ = PC.restated("unshaded")
    assert not flat["dlum"].any() and not np.array_equal(flat["L6"], out["L6"])
    out3, _ = PC.restated("three_poses")
    assert out3["L6"].shape == (3, 6, 6) and not np.array_equal(out3["L6"][0], out3["L6"][1])
    assert np.array_equal(out3["J"][0], out["J"][0])   # the same first pose: J does not read the evidence's settings
    _, cc = PC.restated("cap16")
    assert cc[0]["cut"] > 0
    _, cs = PC.restated("stack")
    assert cs[0]["stopped"] > 0 and cs[0]["alpha_capped"] > 0
    outi, _ = PC.restated("invalid")
    for r in CC.INVALID_ROWS:
        assert outi["lum"][0, r] == 0.0 and not outi["dlum"][0, r].any()
    assert outi["dlum"][0, 0].any() and outi["lum"][0, 0] > 0
    # the background is not read: the same bytes as the zero background
    outb, _ = PC.restated("background")
    assert PC.build("background")["cfg"]["background"] != (0.0, 0.0, 0.0)
    for k in ("L6", "h6", "parts", "residual", "weight", "lum_render"):
        assert outb[k].tobytes() == out[k].tobytes(), k
    c8 = PC.build("rgb8")
    assert c8["image_obs"].dtype == np.uint8 and c8["image_obs"].shape == (32, 32, 3) and c8["lum_obs"].dtype == np.float32
    out8, _ = PC.restated("rgb8")
    assert out8["n_used"][0] == out["n_used"][0] and 0 < np.max(np.abs(out8["residual"] - out["residual"])) < 1.0 / 255.0
    outh, _ = PC.restated("holes")
    holes = ~np.isfinite(PC.build("holes")["lum_obs"])
    assert holes.sum() >= 7 and not outh["used"][0][holes].any()
    assert not outh["residual"][0][holes].any() and not outh["weight"][0][holes].any()
    assert outh["n_used"][0] == out["n_used"][0] - int((holes & out["used"][0]).sum()) < out["n_used"][0]
    for name in ("all_nan", "empty"):
        o, _ = PC.restated(name)
        assert o["n_used"][0] == 0 and not o["L6"].any() and not o["h_pose"].any() and not o["parts"].any()
        assert np.array_equal(o["L_pose"][0, :6, :6], 1e-9 * np.eye(6))
    o8, _ = PC.restated("ts8")
    assert PC.build("ts8")["cfg"]["tile_size"] == 8 and o8["n_used"][0] > 0
    ow, _ = PC.restated("weights")
    assert PC.build("weights")["pcfg"]["weights"] == (0.5, -0.25, 1.0) and not np.array_equal(ow["lum"], out["lum"])
    assert ow["n_used"][0] == out["n_used"][0]


# ------------------------------------------------------------------------------------- argument errors
K_OK = PinholeIntrinsics(fx=60.0, fy=60.0, cx=16.0, cy=16.0)
Y_OK = np.full((32, 32), 0.5, np.float32)
RGB_OK = np.zeros((32, 32, 3), np.uint8)
D_OK = np.ones((32, 32), np.float32)
P_OK = np.zeros((1, 6))
BAD = [
    (dict(poses6=np.zeros((33, 6))), "poses"),
    (dict(poses6=np.zeros((0, 6))), "poses"),
    (dict(poses6=np.zeros((2, 5))), "poses6"),
    (dict(poses6=np.array([[0, 0, 0, 0, np.nan, 0.0]])), "finite"),
    (dict(view_cfg=CameraViewConfig(tile_size=32)), "tile_size"),
    (dict(image_obs=np.ones((32, 32, 1), np.uint8)), "image_obs"),
    (dict(image_obs=np.ones((32, 32, 3), np.float32)), "uint8"),
    (dict(image_obs=np.ones((32, 32), np.uint8)), "float"),
    (dict(image_obs=np.ones((30, 32), np.float32)), "multiple of tile_size"),
    (dict(image_obs=np.ones((32,), np.float32)), "image_obs"),
    (dict(R_base_camera=np.eye(3) * 1.1), "rotation"),
    (dict(R_base_camera=np.eye(4)), "R_base_camera"),
    (dict(t_base_camera=[0.0, np.inf, 0.0]), "finite"),
    (dict(cfg=PhotometricEvidenceConfig(sigma=0.0)), "sigma"),
    (dict(cfg=PhotometricEvidenceConfig(sigma=-1.0)), "sigma"),
    (dict(cfg=PhotometricEvidenceConfig(sigma=np.nan)), "finite"),
    (dict(cfg=PhotometricEvidenceConfig(robust_nu=0.0)), "robust_nu"),
    (dict(cfg=PhotometricEvidenceConfig(eps_lift=-1.0)), "eps_lift"),
    (dict(cfg=PhotometricEvidenceConfig(weights=(1.0, 2.0))), "weights"),
    (dict(cfg=PhotometricEvidenceConfig(weights=(1.0, np.inf, 0.0))), "weights"),
    (dict(intrinsics=(60.0, 60.0, 16.0, 16.0)), "PinholeIntrinsics"),
    (dict(accumulate_into=(np.zeros((1, 22, 22)), np.zeros((1, 22)))), "accumulate_into"),
]


@pytest.mark.parametrize("kw, word", BAD)
def test_wrapper_refuses_before_a_device(kw, word):
    """The batch argument is checked last, so an object that is no batch shows that no device was asked for."""
    args = dict(intrinsics=K_OK, poses6=P_OK, image_obs=Y_OK)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        photometric_pose_evidence_batched(object(), **args)
    for ok in (Y_OK, RGB_OK):
        with pytest.raises(ValueError, match="cannot render"):
            photometric_pose_evidence_batched(object(), K_OK, P_OK, ok)


@pytest.mark.parametrize("kw, word", [(dict(photo_cfg=k["cfg"]) if "cfg" in k else k, w) for k, w in BAD] + [
    (dict(depth_obs=np.ones((48, 64), np.float32)), "beside depth_obs"),
    (dict(depth_obs=np.ones((32, 32, 1), np.float32)), "depth_obs"),
    (dict(depth_cfg=DepthEvidenceConfig(depth_sigma0=0.0)), "depth_sigma0"),
    (dict(depth_cfg=DepthEvidenceConfig(eps_lift=1e-6)), "eps_lift"),
    (dict(image_obs=None), "both"),
])
def test_joint_wrapper_refuses_before_a_device(kw, word):
    args = dict(intrinsics=K_OK, poses6=P_OK, depth_obs=D_OK, image_obs=Y_OK)
    args.update(kw)
    if np.ndim(kw.get("image_obs")) == 2 and "depth_obs" not in kw:
        args["depth_obs"] = np.ones(np.shape(kw["image_obs"]), np.float32)   # a frame of the image's size
    with pytest.raises(ValueError, match=word):
        rgbd_pose_evidence_batched(object(), **args)
    with pytest.raises(ValueError, match="cannot render"):
        rgbd_pose_evidence_batched(object(), K_OK, P_OK, D_OK, RGB_OK)


@pytest.mark.parametrize("kw, word", [(dict(rgb=Y_OK), "rgb"), (dict(rgb=np.zeros((32, 32, 3), np.float32)), "uint8"),
                                      (dict(weights=(1.0, np.nan, 0.0)), "weights"), (dict(weights=(1.0,)), "weights")])
def test_luminance_image_refuses_before_a_device(kw, word):
    args = dict(rgb=RGB_OK, ctx=object())
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        luminance_image(**args)


@pytest.mark.parametrize("module, operator, trigger, cls", [
    ("depth_pose_evidence", "depth_pose_evidence", "render_depth_residual", "DepthPoseEvidenceResult"),
    ("photometric_pose_evidence", "photometric_pose_evidence", "render_photometric_residual", "PhotometricPoseEvidenceResult")])
def test_result_from_parts_reads_a_parts_row(module, operator, trigger, cls):
    """Both result_from_parts on synthetic 46-value rows [L6 (36) | h6 (6) | cost | n_used | sum_cov | sum_w]: the
    fields come from the documented offsets, the certificate is approximate with the operator's own residual
    trigger, and exact with a zero effect when no pixel is used; the anchor and the objective are the operator's."""
    import importlib
    import gcslam.ops
    mod = importlib.import_module("gcslam.ops." + module)
    row = np.random.default_rng(9).normal(size=46)
    assert row.shape == (46,)
    row[42:46] = 3.25, 200.0, 150.5, 180.25
    L, h = np.ones((22, 22)), np.ones(22)
    res, cert, eff = mod.result_from_parts(L, h, row, (16, 32), 1e-7, "chart")
    assert type(res) is getattr(gcslam.ops, cls) is getattr(mod, cls)
    assert res.L_pose is L and res.h_pose is h
    assert np.array_equal(res.L6, row[:36].reshape(6, 6)) and np.array_equal(res.h6, row[36:42])
    assert (res.total_weighted_cost, res.n_used, res.sum_coverage, res.sum_weight) == (3.25, 200, 150.5, 180.25)
    assert isinstance(res.n_used, int)
    assert not cert.exact and cert.approximation_triggers == ["linearization", trigger]
    assert cert.chart_id == "chart" and cert.anchor_id == operator
    assert cert.support.support_frac == 200 / (16 * 32.0) and cert.support.ess_total == 150.5
    assert cert.influence.lift_strength == 1e-7
    assert eff.objective_name == operator and eff.predicted == eff.realized == 3.25
    row[0] = 7.0   # the results hold copies of the row
    assert res.L6[0, 0] != 7.0
    _, cert_a, _ = mod.result_from_parts(None, None, row, (16, 32), anchor_id="elsewhere")
    assert cert_a.anchor_id == "elsewhere"
    row[43] = 0.0
    res0, cert0, eff0 = mod.result_from_parts(None, None, row, (16, 32))
    assert res0.n_used == 0 and cert0.exact and cert0.anchor_id == operator
    assert eff0.objective_name == operator and eff0.predicted == 0.0 and eff0.realized == 0.0
