"""The photometric pose evidence on the device (csrc/gc_depthev.hip, gcslam/ops/photometric_pose_evidence.py)
against the restatement (tests/photoev_restatement.py) on the seeded cases (tests/photoev_cases.py), whose
conditions tests/test_photo_evidence.py asserts.

Exact: n_used and n_contrib, the bytes of the joint entry against the two single entries. Float fields:
max |difference| over the field <= 1e-10 of the field's max-abs over the case (camrender_cases.err_frac, the
camera view's bar). The measured worst fractions are printed and recorded in DESIGN.md §4."""

import ctypes

import numpy as np
import pytest

import camrender_cases as CC
import photoev_cases as PC
import photoev_restatement as PS
from gcslam import _abi
from gcslam import rendering as R
from gcslam.ops import (DepthEvidenceConfig, PhotometricEvidenceConfig, PinholeIntrinsics, depth_pose_evidence_batched,
                        luminance_image, photometric_pose_evidence, photometric_pose_evidence_batched,
                        rgbd_pose_evidence_batched)
from test_gpu_depth_evidence import _device_batch

pytestmark = pytest.mark.gpu

BAR = 1e-10
FIELDS = ("lum", "dlum", "lum_render", "residual", "weight")


def _cfgs(c):
    return R.CameraViewConfig(**c["cfg"]), PhotometricEvidenceConfig(**c["pcfg"]), DepthEvidenceConfig(**c["ecfg"])


def _run(ctx, name, poses=None, image=None, **kw):
    c = PC.build(name)
    vcfg, pcfg, _ = _cfgs(c)
    poses = c["poses6"] if poses is None else poses
    image = c["image_obs"] if image is None else image
    Lp, hp, parts, render = photometric_pose_evidence_batched(_device_batch(ctx, c["batch"]), PinholeIntrinsics(*c["K"]), poses,
                                                              image, c["R_bc"], c["t_bc"], vcfg, pcfg, return_images=True, **kw)
    out = {k: render[k].download() for k in FIELDS + ("alpha", "n_contrib", "lum_obs", "tile_indices", "tile_counts")}
    return dict(out, L_pose=np.asarray(Lp), h_pose=np.asarray(hp), parts=parts)


_shared = {}


def _once(ctx, name):
    """A case's device outputs, computed once and shared (read-only) by the tests that compare against them."""
    if name not in _shared:
        _shared[name] = _run(ctx, name)
    return _shared[name]


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_gpu_photo_evidence_parity(ctx, name):
    c = PC.build(name)
    want, _ = PC.restated(name)
    got = _once(ctx, name)
    P = c["poses6"].shape[0]
    parts = got["parts"]
    assert parts.shape == (P, _abi.GC_DEPTHEV_PARTS)
    # ---- exact
    np.testing.assert_array_equal(parts[:, 43], want["n_used"].astype(np.float64))
    np.testing.assert_array_equal(got["n_contrib"], want["n_contrib"])
    assert got["lum_obs"].tobytes() == c["lum_obs"].tobytes() or name == "rgb8"
    used = want["used"]
    assert not got["residual"][~used].any() and not got["weight"][~used].any()
    assert (got["weight"][used] > 0).all()
    assert not got["lum_render"][~(got["alpha"] > c["cfg"]["eps"])].any()
    # ---- the parts row against L_pose / h_pose
    L6 = parts[:, :36].reshape(P, 6, 6)
    assert np.array_equal(L6, np.swapaxes(L6, 1, 2))
    eps = c["pcfg"]["eps_lift"]
    assert np.array_equal(got["L_pose"][:, :6, :6], L6 + eps * np.eye(6)) and np.array_equal(got["h_pose"][:, :6], parts[:, 36:42])
    rest = got["L_pose"].copy()
    rest[:, :6, :6] = 0.0
    assert not rest.any() and not got["h_pose"][:, 6:].any()
    # ---- float fields
    worst = {k: CC.err_frac(got[k], want[k]) for k in FIELDS}
    worst.update(L6=CC.err_frac(L6, want["L6"]), h6=CC.err_frac(parts[:, 36:42], want["h6"]),
                 cost=CC.err_frac(parts[:, 42], want["cost"]), sum_cov=CC.err_frac(parts[:, 44], want["sum_cov"]),
                 sum_w=CC.err_frac(parts[:, 45], want["sum_w"]))
    print(name, "worst difference / max-abs:", {k: float("%.3g" % v) for k, v in worst.items()})
    assert max(worst.values()) <= BAR, worst
    if not want["n_used"].any():  # the exact certificate's evidence
        assert not parts.any()


def test_gpu_background_is_not_read(ctx):
    """A nonzero background gives the zero background's bytes."""
    a, b = _once(ctx, "shaded"), _once(ctx, "background")
    for k in ("L_pose", "h_pose", "parts", "lum_render", "residual", "weight"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_gpu_image_luminance(ctx):
    """gc_image_luminance against NumPy's same expression, within one float32 ulp; the rgb8 case observes it;
    a device image is read in place."""
    rng = np.random.default_rng(31)
    rgb = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    rgb[0, 0], rgb[0, 1] = 0, 255
    for w in (PS.GREY, (0.5, -0.25, 1.0)):
        want = PS.image_luminance(rgb, w)
        got = luminance_image(rgb, None if w is PS.GREY else w, ctx=ctx)
        assert got.dtype == np.float32 and got.shape == (48, 64)
        assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))).all()
        dev = luminance_image(_abi.DeviceArray.from_host(ctx, rgb, np.uint8), None if w is PS.GREY else w, device_out=True)
        assert dev.download().tobytes() == got.tobytes()
    c = PC.build("rgb8")
    got = _once(ctx, "rgb8")["lum_obs"]
    assert (np.abs(got.astype(np.float64) - c["lum_obs"]) <= np.spacing(np.abs(c["lum_obs"]))).all()
    lum = _run(ctx, "rgb8", image=got)   # the float image the device made gives the rgb8 call's bytes
    for k in ("L_pose", "h_pose", "parts"):
        assert lum[k].tobytes() == _once(ctx, "rgb8")[k].tobytes(), k


# ------------------------------------------------------------------------------------- joint against single
def _joint(ctx, name, joint, image=None, **kw):
    c = PC.build(name)
    vcfg, pcfg, dcfg = _cfgs(c)
    image = c["image_obs"] if image is None else image
    Lp, hp, parts, render = rgbd_pose_evidence_batched(_device_batch(ctx, c["batch"]), PinholeIntrinsics(*c["K"]), c["poses6"],
                                                       PC.depth_obs(name), image, c["R_bc"], c["t_bc"], vcfg, dcfg, pcfg,
                                                       return_images=True, joint=joint, **kw)
    out = {k: render[k].download() for k in ("residual", "weight", "lum_render", "lum_residual", "lum_weight")}
    return dict(out, L_pose=np.asarray(Lp), h_pose=np.asarray(hp), parts=parts)


def _depth_alone(ctx, name, **kw):
    c = PC.build(name)
    vcfg, _, dcfg = _cfgs(c)
    Lp, hp, parts, render = depth_pose_evidence_batched(_device_batch(ctx, c["batch"]), PinholeIntrinsics(*c["K"]), c["poses6"],
                                                        PC.depth_obs(name), c["R_bc"], c["t_bc"], vcfg, dcfg,
                                                        return_images=True, **kw)
    return dict(L_pose=np.asarray(Lp), h_pose=np.asarray(hp), parts=parts, residual=render["residual"].download(),
                weight=render["weight"].download())


@pytest.mark.parametrize("name", ["three_poses", "cap16", "stack"])
def test_gpu_joint_rows_are_the_single_entries_bytes(ctx, name):
    """The joint entry's depth row is gc_depth_pose_evidence's bytes and its luminance row
    gc_photo_pose_evidence's; L and h are the depth's with the luminance's added; the two-call path of the
    wrapper gives the joint entry's bytes."""
    c = PC.build(name)
    P = c["poses6"].shape[0]
    one, two = _joint(ctx, name, True), _joint(ctx, name, False)
    for k in one:
        assert one[k].tobytes() == two[k].tobytes(), k
    assert one["parts"].shape == (P, 2, _abi.GC_DEPTHEV_PARTS)
    d, y = _depth_alone(ctx, name), _once(ctx, name)
    assert one["parts"][:, 0].tobytes() == d["parts"].tobytes() and one["parts"][:, 1].tobytes() == y["parts"].tobytes()
    assert one["residual"].tobytes() == d["residual"].tobytes() and one["weight"].tobytes() == d["weight"].tobytes()
    for k in ("lum_render", "residual", "weight"):
        assert one[k if k == "lum_render" else "lum_" + k].tobytes() == y[k].tobytes(), k
    wantL, wanth = d["L_pose"].copy(), d["h_pose"].copy()   # the depth's, lift included, then one addition
    wantL[:, :6, :6] += y["parts"][:, :36].reshape(P, 6, 6)
    wanth[:, :6] += y["parts"][:, 36:42]
    assert one["L_pose"].tobytes() == wantL.tobytes() and one["h_pose"].tobytes() == wanth.tobytes()
    # without luminance (every pixel a hole) L and h are the depth entry's bytes
    none = _joint(ctx, name, True, image=np.full((c["H"], c["W"]), np.nan, np.float32))
    assert none["L_pose"].tobytes() == d["L_pose"].tobytes() and none["h_pose"].tobytes() == d["h_pose"].tobytes()
    assert none["parts"][:, 0].tobytes() == d["parts"].tobytes() and not none["parts"][:, 1].any()


def test_gpu_joint_accumulation_is_the_two_single_ones_in_order(ctx):
    c = PC.build("three_poses")
    P = c["poses6"].shape[0]
    rng = np.random.default_rng(4)
    L0, h0 = rng.normal(size=(P, 22, 22)) * 100.0, rng.normal(size=(P, 22))
    outs = []
    for joint in (True, False, None):
        dL, dh = _abi.DeviceArray.from_host(ctx, L0), _abi.DeviceArray.from_host(ctx, h0)
        if joint is None:   # by hand: the depth operator, then the photometric operator, into the same arrays
            _depth_alone(ctx, "three_poses", accumulate_into=(dL, dh))
            _run(ctx, "three_poses", accumulate_into=(dL, dh))
        else:
            _joint(ctx, "three_poses", joint, accumulate_into=(dL, dh))
        outs.append((dL.download(), dh.download()))
    for L1, h1 in outs[1:]:
        assert L1.tobytes() == outs[0][0].tobytes() and h1.tobytes() == outs[0][1].tobytes()
    assert not np.array_equal(outs[0][0][:, :6, :6], L0[:, :6, :6])


def test_gpu_evidence_gives_the_recorded_bytes(ctx):
    """The photometric and the joint routes, and accumulate_into and device_out on the three routes: the bytes the
    build gave while depth_pose_evidence.py and photometric_pose_evidence.py each held their own host driver
    (tests/golden/evidence_parent.npz, recorded by make_evidence_parent.py before they became
    camview_pose_evidence.py's). L_pose, h_pose and parts byte for byte, the per-splat arrays and the images by
    their SHA-256."""
    from tests.golden import make_evidence_parent as MP
    gold = np.load(MP.OUT)
    seen = set()
    for route, name in MP.RUNS:
        got = MP.run(ctx, route, name)
        digests = got.pop("sha256")
        want = gold[f"{route}/{name}/sha256"]
        kind = MP.DEPTH_DIGESTS if route == "acc_depth" else MP.PHOTO_DIGESTS if route.endswith("photo") else MP.JOINT_DIGESTS
        assert want.shape == digests.shape == (len(kind), 32)
        for k, a, b in zip(kind, digests, want):
            assert a.tobytes() == b.tobytes(), (route, name, k)
        for k, a in got.items():
            assert MP.same_as_recorded(gold, f"{route}/{name}/{k}", a), (route, name, k)
        seen.update(f"{route}/{name}/{k}" for k in list(got) + ["sha256"])
    assert seen == set(gold.files) and len(seen) == 18 * 4


# ------------------------------------------------------------------------------------------ reproducibility
def test_gpu_photo_evidence_reproducible_and_rows(ctx):
    """Two calls give identical bytes; a row of the batched call is the single call for that pose; a device
    pose array equals a host one."""
    a, b = _once(ctx, "three_poses"), _run(ctx, "three_poses")
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    poses = PC.build("three_poses")["poses6"]
    for p in range(poses.shape[0]):
        one = _run(ctx, "three_poses", poses=poses[p:p + 1])
        for k in a:
            if k != "lum_obs":
                assert one[k][0].tobytes() == a[k][p].tobytes(), (p, k)
    d = _run(ctx, "three_poses", poses=_abi.DeviceArray.from_host(ctx, poses))
    for k in a:
        assert a[k].tobytes() == d[k].tobytes(), k


def test_gpu_photo_evidence_operator(ctx):
    c = PC.build("shaded")
    vcfg, pcfg, _ = _cfgs(c)
    K = PinholeIntrinsics(*c["K"])
    batch = _device_batch(ctx, c["batch"])
    res, cert, eff = photometric_pose_evidence(batch, K, c["poses6"][0], c["image_obs"], c["R_bc"], c["t_bc"], vcfg, pcfg)
    got = _once(ctx, "shaded")
    assert res.L_pose.tobytes() == got["L_pose"][0].tobytes() and res.h_pose.tobytes() == got["h_pose"][0].tobytes()
    assert res.n_used == 909 and not cert.exact and cert.anchor_id == "photometric_pose_evidence"
    assert cert.approximation_triggers == ["linearization", "render_photometric_residual"]
    assert cert.support.ess_total == res.sum_coverage and cert.support.support_frac == 909 / 1024.0
    assert cert.influence.lift_strength == pcfg.eps_lift
    assert eff.predicted == eff.realized == res.total_weighted_cost > 0.0
    step = np.linalg.solve(res.L6 + 1e-9 * np.eye(6), res.h6)
    assert np.linalg.norm(step - PC.D_STAR) / np.linalg.norm(PC.D_STAR) < 0.1
    res0, cert0, eff0 = photometric_pose_evidence(batch, K, c["poses6"][0], np.full((32, 32), np.nan, np.float32), c["R_bc"],
                                                  c["t_bc"], vcfg, pcfg)
    assert cert0.exact and res0.n_used == 0 and not res0.L6.any() and not res0.h_pose.any() and eff0.predicted == 0.0
    assert np.array_equal(res0.L_pose[:6, :6], pcfg.eps_lift * np.eye(6))


def test_gpu_photo_evidence_accumulates(ctx):
    """accumulate_into adds only the 36 + 6 entries and leaves the rest alone."""
    c = PC.build("three_poses")
    P = c["poses6"].shape[0]
    sep = _once(ctx, "three_poses")
    rng = np.random.default_rng(3)
    L0, h0 = rng.normal(size=(P, 22, 22)) * 100.0, rng.normal(size=(P, 22))
    dL, dh = _abi.DeviceArray.from_host(ctx, L0), _abi.DeviceArray.from_host(ctx, h0)
    acc = _run(ctx, "three_poses", accumulate_into=(dL, dh))
    L1, h1 = dL.download(), dh.download()
    assert acc["L_pose"].tobytes() == L1.tobytes() and acc["h_pose"].tobytes() == h1.tobytes()
    assert acc["parts"].tobytes() == sep["parts"].tobytes()
    L6, h6 = sep["parts"][:, :36].reshape(P, 6, 6), sep["parts"][:, 36:42]
    wantL, wanth = L0[:, :6, :6] + L6, h0[:, :6] + h6
    assert L1[:, :6, :6].tobytes() == wantL.tobytes() and h1[:, :6].tobytes() == wanth.tobytes()
    mask = np.ones((22, 22), bool)
    mask[:6, :6] = False
    assert L1[:, mask].tobytes() == L0[:, mask].tobytes() and h1[:, 6:].tobytes() == h0[:, 6:].tobytes()


# -------------------------------------------------------------------------------------------- bad arguments
def _raw(ctx):
    """Valid raw arguments of the four entries for the `shaded` case, as dicts in argument order."""
    c = PC.build("shaded")
    vcfg, _, _ = _cfgs(c)
    batch = _device_batch(ctx, c["batch"])
    n, H, W = batch.count, c["H"], c["W"]
    T_cw = R.camera_from_world(c["poses6"][0], c["R_bc"], c["t_bc"], ctx=ctx)[None].copy()
    K = np.array([c["K"]], np.float64)
    t_wb = c["poses6"][:1, :3].copy()
    w = np.array(PS.GREY, np.float64)
    splats = R.camera_splat_prep(batch, PinholeIntrinsics(*c["K"]), T_cw, H, W, vcfg)
    dev = R.render_depth_tiles(splats, H, W, vcfg, ctx=ctx)
    st = R._CamSplatStruct(*[splats[k].ptr for k, _ in R._CamSplatStruct._fields_])
    c_cfg = R._camview_cfg(vcfg)
    dm, dz, dS, dl, ddl, dL, dh, dp, dp2 = _abi.alloc_many(ctx, [(1, n, 6, 2), (1, n, 6), (1, n, 6, 3), (1, n), (1, n, 6),
                                                                 (1, 22, 22), (1, 22), (1, 46), (1, 2, 46)])
    obs = _abi.DeviceArray.from_host(ctx, c["lum_obs"], np.float32)
    dobs = _abi.DeviceArray.from_host(ctx, PC.depth_obs("shaded"), np.float32)
    rgb = _abi.DeviceArray.from_host(ctx, PC.build("rgb8")["image_obs"], np.uint8)
    lum8 = _abi.DeviceArray(ctx, (H, W), np.float32)
    keep = (batch, splats, dev, st, c_cfg, T_cw, K, t_wb, w, obs, dobs, rgb, lum8, dm, dz, dS, dl, ddl, dL, dh, dp, dp2)
    view = dict(batch=ctypes.byref(batch.struct), n=n, n_poses=1, T=T_cw.ctypes.data, t_wb=t_wb.ctypes.data, K=K.ctypes.data,
                H=H, W=W, cfg=ctypes.byref(c_cfg), splats=ctypes.byref(st))
    jvp = dict(view, dm=dm.ptr, dz=dz.ptr, dS=dS.ptr)
    shade = dict(view, w=w.ctypes.data, lum=dl.ptr, dlum=ddl.ptr)
    frame = dict(H=H, W=W, ts=16, cap=256, cfg=ctypes.byref(c_cfg), counts=dev["tile_counts"].ptr,
                 indices=dev["tile_indices"].ptr, alpha=dev["alpha"].ptr)
    ev = dict(n_poses=1, n=n, splats=ctypes.byref(st), dm=dm.ptr, dS=dS.ptr, lum=dl.ptr, dlum=ddl.ptr, **frame, obs=obs.ptr,
              sigma=0.05, robust=1, nu=4.0, eps_lift=1e-9, accumulate=0, L=dL.ptr, h=dh.ptr, parts=dp.ptr, render=None, res=None,
              w=None)
    rgbd = dict(n_poses=1, n=n, splats=ctypes.byref(st), dm=dm.ptr, dz=dz.ptr, dS=dS.ptr, lum=dl.ptr, dlum=ddl.ptr, **frame,
                depth=dev["depth"].ptr, dobs=dobs.ptr, model=0, sigma0=0.01, slope=0.01, dmin=0.05, dmax=50.0, drobust=1, dnu=4.0,
                obs=obs.ptr, sigma=0.05, robust=1, nu=4.0, eps_lift=1e-9, accumulate=0, L=dL.ptr, h=dh.ptr, parts=dp2.ptr,
                res=None, w=None, render=None, lres=None, lw=None)
    img = dict(rgb=rgb.ptr, H=H, W=W, w=w.ctypes.data, lum=lum8.ptr)
    return keep, jvp, shade, ev, rgbd, img


def test_gpu_photo_evidence_refuses_bad_arguments(ctx):
    """Every bad raw argument is GC_ERR_ARG (a ValueError) before a launch, and the context stays usable: the
    valid calls afterwards give the bytes they gave before."""
    keep, jvp, shade, ev, rgbd, img = _raw(ctx)
    dp, dp2, lum8 = keep[-2], keep[-1], keep[12]
    call = lambda name, args: _abi.call(name, ctx.handle, *args.values(), ctx=ctx)

    def run():
        call("gc_camera_splat_jvp", jvp)
        call("gc_camera_shade_jvp", shade)
        call("gc_photo_pose_evidence", ev)
        call("gc_rgbd_pose_evidence", rgbd)
        call("gc_image_luminance", img)
        return dp.download().tobytes() + dp2.download().tobytes() + lum8.download().tobytes()

    before = run()
    assert dp2.download()[0, 1].tobytes() == dp.download()[0].tobytes()
    T_bad, T_nan, t_nan = keep[5].copy(), keep[5].copy(), keep[7].copy()
    T_bad[0, :3, :3] *= 1.001
    T_nan[0, 0, 3] = np.nan
    t_nan[0, 1] = np.inf
    w_nan = np.array([0.3, np.nan, 0.1])
    for bad in (dict(n_poses=0), dict(n_poses=33), dict(n=-1), dict(T=T_bad.ctypes.data), dict(T=T_nan.ctypes.data),
                dict(t_wb=t_nan.ctypes.data), dict(H=0), dict(lum=None), dict(dlum=None), dict(splats=None), dict(w=None),
                dict(w=w_nan.ctypes.data), dict(cfg=None), dict(batch=None)):
        with pytest.raises(ValueError):
            call("gc_camera_shade_jvp", dict(shade, **bad))
    common = (dict(n_poses=0), dict(n_poses=33), dict(ts=32), dict(ts=17, H=34, W=34), dict(ts=0), dict(H=30), dict(cap=0),
              dict(cap=257), dict(n=-1), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=np.nan), dict(sigma=np.inf),
              dict(nu=0.0), dict(nu=-4.0), dict(nu=np.nan), dict(eps_lift=-1.0), dict(eps_lift=np.nan), dict(L=None),
              dict(h=None), dict(parts=None), dict(obs=None), dict(dS=None), dict(dm=None), dict(lum=None), dict(dlum=None),
              dict(cfg=None), dict(counts=None), dict(indices=None), dict(alpha=None), dict(splats=None))
    for bad in common:
        with pytest.raises(ValueError):
            call("gc_photo_pose_evidence", dict(ev, **bad))
    for bad in common + (dict(model=2), dict(sigma0=0.0), dict(slope=-0.1), dict(dnu=0.0), dict(dnu=np.nan),
                         dict(dmin=5.0, dmax=5.0), dict(dmax=np.inf), dict(dz=None), dict(depth=None), dict(dobs=None)):
        with pytest.raises(ValueError):
            call("gc_rgbd_pose_evidence", dict(rgbd, **bad))
    for bad in (dict(rgb=None), dict(lum=None), dict(w=None), dict(w=w_nan.ctypes.data), dict(H=0), dict(W=16385)):
        with pytest.raises(ValueError):
            call("gc_image_luminance", dict(img, **bad))
    assert run() == before
    # the wrapper refuses a device pose array that is not finite, and the context stays usable
    poses = PC.build("shaded")["poses6"].copy()
    poses[0, 4] = np.nan
    with pytest.raises(ValueError, match="finite"):
        _run(ctx, "shaded", poses=_abi.DeviceArray.from_host(ctx, poses))
    assert run() == before


# ------------------------------------------------------------------------------------------- the step
def _rgb_frame():
    from test_gpu_depth_evidence import _frame
    rng = np.random.default_rng(6)
    return dict(_frame(), rgb=rng.integers(40, 200, (32, 32, 3), dtype=np.uint8),
                photo_cfg=PhotometricEvidenceConfig(robust_nu=4.0, sigma=0.1))


def test_step_with_rgb_runs_on_front_plus_depth_plus_luminance(ctx):
    """With rgb in the frame the evidence the back ran on is the front's plus the depth and the photometric
    evidence of every hypothesis's linearisation pose, and the photometric certificate follows the depth one."""
    from gcslam.primitive_step import lidar_cert_row, visual_cert
    from test_gpu_depth_evidence import _step_setup
    step, br2, p1, p2, dm1, dm2, meas, s, MC = _step_setup(ctx)
    frame = _rgb_frame()
    r = step.run(0, s, MC.SCAN_SEQ, MC.TIMESTAMP, measurement_batch=meas, depth_frame=frame)
    gl, gh, gc = p1.lidar_evidence()
    p2.stage_scan(0, s)
    p2.scan_front(0, s, MC.SCAN_SEQ)
    lin = p2.front_poses()[0]
    assert lin.tobytes() == p1.front_poses()[0].tobytes()
    front = br2.front(meas, p2.front_poses()[1][0, 0:3], lin, MC.SCAN_SEQ)
    where = (dm2, frame["intrinsics"], lin)
    camera = (None, frame["t_base_camera"], frame["view_cfg"])
    _, _, pd, _ = depth_pose_evidence_batched(*where, frame["depth"], *camera, frame["cfg"])
    _, _, py, _ = photometric_pose_evidence_batched(*where, frame["rgb"], *camera, frame["photo_cfg"])
    p2.set_lidar_evidence(front.L_lidar, front.h_lidar, np.zeros(6))
    p2.scan_back()
    p2.finish_scan()
    assert (pd[:, 43] > 50).all() and (py[:, 43] > 50).all(), (pd[:, 43], py[:, 43])
    assert r.depth_parts.tobytes() == pd.tobytes() and r.photo_parts.tobytes() == py.tobytes()
    wantL, wanth = front.L_lidar.copy(), front.h_lidar.copy()
    for parts in (pd, py):
        wantL[:, :6, :6] += parts[:, :36].reshape(-1, 6, 6)
        wanth[:, :6] += parts[:, 36:42]
    assert np.max(np.abs(gl - wantL)) <= 1e-15 * np.max(np.abs(wantL))
    assert np.max(np.abs(gh - wanth)) <= 1e-15 * np.max(np.abs(wanth))
    assert len(r.certs) == 5 and [x.anchor_id for x in r.certs[-2:]] == ["depth_pose_evidence", "photometric_pose_evidence"]
    assert not r.certs[-1].exact
    row = lidar_cert_row([front.certs[1], visual_cert(front.vpe_cert, br2.config.eps_lift, br2.chart_id)] + r.certs[-2:],
                         [front.certs[0]])
    assert r.lidar_cert.tobytes() == row.tobytes() and gc.tobytes() == np.tile(row, (2, 1)).tobytes()
    assert np.all(np.isfinite(p1.get_beliefs()["L"]))


def test_step_without_rgb_is_the_depth_only_step(ctx):
    """A frame without rgb or luminance: the bytes of the depth-only step, made by hand on a second pipeline."""
    from test_gpu_depth_evidence import _frame, _step_setup
    step, br2, p1, p2, dm1, dm2, meas, s, MC = _step_setup(ctx)
    frame = _frame()
    r = step.run(0, s, MC.SCAN_SEQ, MC.TIMESTAMP, measurement_batch=meas, depth_frame=frame)
    assert r.photo_parts is None and len(r.certs) == 4
    gl, gh, gc = p1.lidar_evidence()
    p2.stage_scan(0, s)
    p2.scan_front(0, s, MC.SCAN_SEQ)
    lin_d, _ = p2.front_poses(device=True)
    front = br2.front(meas, p2.front_poses()[1][0, 0:3], lin_d, MC.SCAN_SEQ, device_out=True)
    _, _, parts, _ = depth_pose_evidence_batched(dm2, frame["intrinsics"], lin_d, frame["depth"], None, frame["t_base_camera"],
                                                 frame["view_cfg"], frame["cfg"],
                                                 accumulate_into=(front.device["L_lidar"], front.device["h_lidar"]),
                                                 device_out=True)
    assert r.depth_parts.tobytes() == parts.tobytes()
    assert gl.tobytes() == front.device["L_lidar"].download().reshape(gl.shape).tobytes()
    assert gh.tobytes() == front.device["h_lidar"].download().reshape(gh.shape).tobytes()
