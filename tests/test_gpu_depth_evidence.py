"""The depth pose evidence on the device (csrc/gc_depthev.hip, gcslam/ops/depth_pose_evidence.py) against
the restatement (tests/depthev_restatement.py) on the seeded cases (tests/depthev_cases.py), whose
conditions tests/test_depth_evidence.py asserts.

Exact: n_used, the rendered depth and alpha (the bytes render_map_camera gives), the residual image
(depth - depth_obs on the used pixels, zero elsewhere). Float fields: max |difference| over the field
<= 1e-10 of the field's max-abs over the case (camrender_cases.err_frac, the camera view's bar). The
measured worst fractions are printed and recorded in DESIGN.md §4."""

import ctypes

import numpy as np
import pytest

import camrender_cases as CC
import depthev_cases as DC
from gcslam import _abi
from gcslam import rendering as R
from gcslam.ops import DepthEvidenceConfig, PinholeIntrinsics, depth_pose_evidence, depth_pose_evidence_batched

pytestmark = pytest.mark.gpu

BAR = 1e-10
TANGENTS = ("dmeans_px", "ddepths", "dSigmas_inv")
IMAGES = ("depth", "alpha", "residual", "weight")


def _device_batch(ctx, b):
    if b["mu_world"].shape[0] == 0:
        return R.DeviceRenderableBatch(ctx, 4, CC.L)   # count = 0: no row is read
    return R.DeviceRenderableBatch.from_host(ctx, R.RenderablePrimitiveBatch(
        mu_world=b["mu_world"], Sigma_world=b["Sigma_world"], Lambda_world=None, eta=b["eta"], mass=b["mass"],
        color=b["color"]))


def _cfgs(c):
    return R.CameraViewConfig(**c["cfg"]), DepthEvidenceConfig(**c["ecfg"])


def _run(ctx, name, poses=None, **kw):
    c = DC.build(name)
    vcfg, ecfg = _cfgs(c)
    poses = c["poses6"] if poses is None else poses
    Lp, hp, parts, render = depth_pose_evidence_batched(_device_batch(ctx, c["batch"]), PinholeIntrinsics(*c["K"]), poses,
                                                        c["depth_obs"], c["R_bc"], c["t_bc"], vcfg, ecfg,
                                                        return_images=True, **kw)
    out = {k: render[k].download() for k in TANGENTS + IMAGES + ("n_contrib", "tile_indices", "tile_counts")}
    return dict(out, L_pose=np.asarray(Lp), h_pose=np.asarray(hp), parts=parts)


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_gpu_depth_evidence_parity(ctx, name):
    c = DC.build(name)
    want, _ = DC.restated(name)
    got = _run(ctx, name)
    P = c["poses6"].shape[0]
    parts = got["parts"]
    assert parts.shape == (P, _abi.GC_DEPTHEV_PARTS)
    # ---- exact
    np.testing.assert_array_equal(parts[:, 43], want["n_used"].astype(np.float64))
    np.testing.assert_array_equal(got["n_contrib"], want["n_contrib"])
    vcfg, _ = _cfgs(c)
    if c["batch"]["mu_world"].shape[0]:
        T_cw = np.stack([R.camera_from_world(p, c["R_bc"], c["t_bc"], ctx=ctx) for p in c["poses6"]])
        ref = R.render_map_camera(_device_batch(ctx, c["batch"]), [PinholeIntrinsics(*c["K"])] * P, T_cw, c["H"], c["W"],
                                  vcfg)
        assert ref.depth.tobytes() == got["depth"].tobytes() and ref.alpha.tobytes() == got["alpha"].tobytes()
    obs = np.asarray(c["depth_obs"], np.float64)
    used = want["used"]
    assert np.array_equal(got["residual"][used], (got["depth"] - obs[None])[used])
    assert not got["residual"][~used].any() and not got["weight"][~used].any()
    assert (got["weight"][used] > 0).all()
    # ---- the parts row against L_pose / h_pose
    L6 = parts[:, :36].reshape(P, 6, 6)
    assert np.array_equal(L6, np.swapaxes(L6, 1, 2))
    eps = c["ecfg"]["eps_lift"]
    assert np.array_equal(got["L_pose"][:, :6, :6], L6 + eps * np.eye(6)) and np.array_equal(got["h_pose"][:, :6], parts[:, 36:42])
    rest = got["L_pose"].copy()
    rest[:, :6, :6] = 0.0
    assert not rest.any() and not got["h_pose"][:, 6:].any()
    # ---- float fields
    worst = {k: CC.err_frac(got[k], want[k]) for k in TANGENTS + ("weight", "residual")}
    worst.update(L6=CC.err_frac(L6, want["L6"]), h6=CC.err_frac(parts[:, 36:42], want["h6"]),
                 cost=CC.err_frac(parts[:, 42], want["cost"]), sum_cov=CC.err_frac(parts[:, 44], want["sum_cov"]),
                 sum_w=CC.err_frac(parts[:, 45], want["sum_w"]))
    print(name, "worst difference / max-abs:", {k: float("%.3g" % v) for k, v in worst.items()})
    assert max(worst.values()) <= BAR, worst
    if not want["n_used"].any():  # the exact certificate's evidence
        assert not parts.any()


def test_gpu_depth_evidence_reproducible_and_rows(ctx):
    """Two calls give identical bytes; a row of the batched call is the single call for that pose."""
    a, b = _run(ctx, "three_poses"), _run(ctx, "three_poses")
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    poses = DC.build("three_poses")["poses6"]
    for p in range(poses.shape[0]):
        one = _run(ctx, "three_poses", poses=poses[p:p + 1])
        for k in a:
            if k in ("tile_indices", "tile_counts", "n_contrib") or k in TANGENTS + IMAGES + ("L_pose", "h_pose", "parts"):
                assert one[k][0].tobytes() == a[k][p].tobytes(), (p, k)
    # a device pose array is read in place
    d = _run(ctx, "three_poses", poses=_abi.DeviceArray.from_host(ctx, poses))
    for k in a:
        assert a[k].tobytes() == d[k].tobytes(), k


def test_gpu_depth_evidence_operator(ctx):
    c = DC.build("extrinsics")
    vcfg, ecfg = _cfgs(c)
    K = PinholeIntrinsics(*c["K"])
    batch = _device_batch(ctx, c["batch"])
    res, cert, eff = depth_pose_evidence(batch, K, c["poses6"][0], c["depth_obs"], c["R_bc"], c["t_bc"], vcfg, ecfg)
    got = _run(ctx, "extrinsics")
    assert res.L_pose.tobytes() == got["L_pose"][0].tobytes() and res.h_pose.tobytes() == got["h_pose"][0].tobytes()
    assert res.n_used == 909 and not cert.exact
    assert cert.approximation_triggers == ["linearization", "render_depth_residual"]
    assert cert.support.ess_total == res.sum_coverage and cert.support.support_frac == 909 / 1024.0
    assert cert.influence.lift_strength == ecfg.eps_lift
    assert eff.predicted == eff.realized == res.total_weighted_cost > 0.0
    step = np.linalg.solve(res.L6 + 1e-9 * np.eye(6), res.h6)
    assert np.linalg.norm(step - DC.D_STAR) / np.linalg.norm(DC.D_STAR) < 0.1
    res0, cert0, eff0 = depth_pose_evidence(batch, K, c["poses6"][0], np.full((32, 32), np.nan, np.float32), c["R_bc"],
                                            c["t_bc"], vcfg, ecfg)
    assert cert0.exact and res0.n_used == 0 and not res0.L6.any() and not res0.h_pose.any() and eff0.predicted == 0.0
    assert np.array_equal(res0.L_pose[:6, :6], ecfg.eps_lift * np.eye(6))


def test_gpu_depth_evidence_accumulates(ctx):
    """accumulate_into adds L6 and h6 into the caller's arrays on the device and touches nothing else."""
    c = DC.build("three_poses")
    P = c["poses6"].shape[0]
    sep = _run(ctx, "three_poses")
    rng = np.random.default_rng(3)
    L0, h0 = rng.normal(size=(P, 22, 22)) * 100.0, rng.normal(size=(P, 22))
    dL, dh = _abi.DeviceArray.from_host(ctx, L0), _abi.DeviceArray.from_host(ctx, h0)
    acc = _run(ctx, "three_poses", accumulate_into=(dL, dh))
    L1, h1 = dL.download(), dh.download()
    assert acc["L_pose"].tobytes() == L1.tobytes() and acc["h_pose"].tobytes() == h1.tobytes()
    assert acc["parts"].tobytes() == sep["parts"].tobytes()
    L6, h6 = sep["parts"][:, :36].reshape(P, 6, 6), sep["parts"][:, 36:42]
    wantL, wanth = L0[:, :6, :6] + L6, h0[:, :6] + h6
    assert np.max(np.abs(L1[:, :6, :6] - wantL)) <= 1e-15 * np.max(np.abs(wantL))
    assert np.max(np.abs(h1[:, :6] - wanth)) <= 1e-15 * np.max(np.abs(wanth))
    mask = np.ones((22, 22), bool)
    mask[:6, :6] = False
    assert L1[:, mask].tobytes() == L0[:, mask].tobytes() and h1[:, 6:].tobytes() == h0[:, 6:].tobytes()


def _raw(ctx):
    """Valid raw arguments of the two entries for the `extrinsics` case, as dicts in argument order."""
    c = DC.build("extrinsics")
    vcfg, _ = _cfgs(c)
    batch = _device_batch(ctx, c["batch"])
    n, H, W = batch.count, c["H"], c["W"]
    T_cw = R.camera_from_world(c["poses6"][0], c["R_bc"], c["t_bc"], ctx=ctx)[None].copy()
    K = np.array([c["K"]], np.float64)
    t_wb = c["poses6"][:1, :3].copy()
    splats = R.camera_splat_prep(batch, PinholeIntrinsics(*c["K"]), T_cw, H, W, vcfg)
    dev = R.render_depth_tiles(splats, H, W, vcfg, ctx=ctx)
    st = R._CamSplatStruct(*[splats[k].ptr for k, _ in R._CamSplatStruct._fields_])
    c_cfg = R._camview_cfg(vcfg)
    dm, dz, dS, dL, dh, dp = _abi.alloc_many(ctx, [(1, n, 6, 2), (1, n, 6), (1, n, 6, 3), (1, 22, 22), (1, 22), (1, 46)])
    obs = _abi.DeviceArray.from_host(ctx, c["depth_obs"], np.float32)
    keep = (batch, splats, dev, st, c_cfg, T_cw, K, t_wb, obs, dm, dz, dS, dL, dh, dp)
    jvp = dict(batch=ctypes.byref(batch.struct), n=n, n_poses=1, T=T_cw.ctypes.data, t_wb=t_wb.ctypes.data, K=K.ctypes.data,
               H=H, W=W, cfg=ctypes.byref(c_cfg), splats=ctypes.byref(st), dm=dm.ptr, dz=dz.ptr, dS=dS.ptr)
    ev = dict(n_poses=1, n=n, splats=ctypes.byref(st), dm=dm.ptr, dz=dz.ptr, dS=dS.ptr, H=H, W=W, ts=16, cap=256,
              cfg=ctypes.byref(c_cfg), counts=dev["tile_counts"].ptr, indices=dev["tile_indices"].ptr, alpha=dev["alpha"].ptr,
              depth=dev["depth"].ptr, obs=obs.ptr, model=0, sigma0=0.01, slope=0.01, dmin=0.05, dmax=50.0, robust=1, nu=4.0,
              eps_lift=1e-9, accumulate=0, L=dL.ptr, h=dh.ptr, parts=dp.ptr, res=None, w=None)
    return keep, jvp, ev


def test_gpu_depth_evidence_refuses_bad_arguments(ctx):
    """Every bad argument is GC_ERR_ARG (a ValueError) before a launch, and the context stays usable: the
    valid calls afterwards give the bytes they gave before."""
    keep, jvp, ev = _raw(ctx)
    dp = keep[-1]

    def run():
        _abi.call("gc_camera_splat_jvp", ctx.handle, *jvp.values(), ctx=ctx)
        _abi.call("gc_depth_pose_evidence", ctx.handle, *ev.values(), ctx=ctx)
        return dp.download().tobytes()

    before = run()
    T_bad, T_nan, t_nan = keep[5].copy(), keep[5].copy(), keep[7].copy()
    T_bad[0, :3, :3] *= 1.001
    T_nan[0, 0, 3] = np.nan
    t_nan[0, 1] = np.inf
    for bad in (dict(n_poses=0), dict(n_poses=33), dict(n=-1), dict(T=T_bad.ctypes.data), dict(T=T_nan.ctypes.data),
                dict(t_wb=t_nan.ctypes.data), dict(H=0), dict(dm=None), dict(splats=None)):
        with pytest.raises(ValueError):
            _abi.call("gc_camera_splat_jvp", ctx.handle, *dict(jvp, **bad).values(), ctx=ctx)
    for bad in (dict(n_poses=0), dict(n_poses=33), dict(ts=32), dict(ts=17, H=34, W=34), dict(ts=0), dict(H=30), dict(cap=0),
                dict(cap=257), dict(n=-1), dict(model=2), dict(sigma0=0.0), dict(sigma0=-1.0), dict(slope=-0.1),
                dict(nu=0.0), dict(nu=-4.0), dict(nu=np.nan), dict(dmin=5.0, dmax=5.0), dict(dmin=6.0, dmax=5.0),
                dict(dmax=np.inf), dict(eps_lift=-1.0), dict(sigma0=np.nan), dict(L=None), dict(parts=None), dict(obs=None),
                dict(dS=None), dict(cfg=None)):
        with pytest.raises(ValueError):
            _abi.call("gc_depth_pose_evidence", ctx.handle, *dict(ev, **bad).values(), ctx=ctx)
    assert run() == before
    # the wrapper refuses a device pose array that is not finite, and the context stays usable
    c = DC.build("extrinsics")
    poses = c["poses6"].copy()
    poses[0, 4] = np.nan
    with pytest.raises(ValueError, match="finite"):
        _run(ctx, "extrinsics", poses=_abi.DeviceArray.from_host(ctx, poses))
    assert run() == before


# ------------------------------------------------------------------------------------------- the step
def _frame():
    return dict(depth=np.full((32, 32), 9.0, np.float32), intrinsics=PinholeIntrinsics(40.0, 40.0, 16.0, 16.0),
                t_base_camera=np.array([0.0, 0.0, -9.0]), view_cfg=R.CameraViewConfig(max_splats_per_tile=64),
                cfg=DepthEvidenceConfig(robust_nu=4.0, depth_sigma0=0.05))


def _step_setup(ctx):
    from gcslam.map_branch import MapBranch
    from gcslam.primitive_step import PrimitiveScanStep
    from test_gpu_mapbranch import _branch_config
    from test_gpu_mapupdate import _Obj, _fresh_map
    from test_gpu_primstep import _pipe, _step_case
    import mapupdate_cases as MC
    mcase = MC.build("ragged")
    cfg = _branch_config(mcase["m_view"], mcase["K"], mcase["k_ins"])
    case = _step_case(1)
    dm1, dm2 = _fresh_map(ctx, mcase), _fresh_map(ctx, mcase)
    p1, p2 = _pipe(case, ctx, False), _pipe(case, ctx, True)
    return (PrimitiveScanStep(p1, MapBranch(dm1, cfg)), MapBranch(dm2, cfg), p1, p2, dm1, dm2, _Obj(**mcase["meas"]),
            case["scans"][0], MC)


def test_step_without_a_frame_is_unchanged(ctx):
    """depth_frame=None: the bytes of the calls the step made before it took a frame, made by hand."""
    from test_gpu_primstep import _by_hand, _same_step
    step, br2, p1, p2, dm1, dm2, meas, s, MC = _step_setup(ctx)
    r = step.run(0, s, MC.SCAN_SEQ, MC.TIMESTAMP, measurement_batch=meas, depth_frame=None)
    _same_step(r, _by_hand(p2, br2, s, MC.SCAN_SEQ, MC.TIMESTAMP, meas=meas), p1, p2, dm1, dm2)
    assert r.depth_parts is None and len(r.certs) == 3


def test_step_with_a_frame_runs_on_front_plus_depth(ctx):
    """With a frame the evidence the back ran on is the front's plus the depth evidence of every
    hypothesis's linearisation pose, and its certificate joins the evidence certificates."""
    from gcslam.primitive_step import lidar_cert_row, visual_cert
    step, br2, p1, p2, dm1, dm2, meas, s, MC = _step_setup(ctx)
    frame = _frame()
    r = step.run(0, s, MC.SCAN_SEQ, MC.TIMESTAMP, measurement_batch=meas, depth_frame=frame)
    gl, gh, gc = p1.lidar_evidence()
    # by hand on the second map and pipeline: the front alone, then the depth evidence on its own
    p2.stage_scan(0, s)
    p2.scan_front(0, s, MC.SCAN_SEQ)
    lin = p2.front_poses()[0]
    assert lin.tobytes() == p1.front_poses()[0].tobytes()
    front = br2.front(meas, p2.front_poses()[1][0, 0:3], lin, MC.SCAN_SEQ)
    Ld, hd, parts, _ = depth_pose_evidence_batched(dm2, frame["intrinsics"], lin, frame["depth"], None,
                                                   frame["t_base_camera"], frame["view_cfg"], frame["cfg"])
    p2.set_lidar_evidence(front.L_lidar, front.h_lidar, np.zeros(6))
    p2.scan_back()
    p2.finish_scan()
    assert (parts[:, 43] > 50).all(), parts[:, 43]
    assert r.depth_parts.tobytes() == parts.tobytes()
    L6, h6 = parts[:, :36].reshape(-1, 6, 6), parts[:, 36:42]
    wantL, wanth = front.L_lidar.copy(), front.h_lidar.copy()
    wantL[:, :6, :6] += L6
    wanth[:, :6] += h6
    assert np.max(np.abs(gl - wantL)) <= 1e-15 * np.max(np.abs(wantL))
    assert np.max(np.abs(gh - wanth)) <= 1e-15 * np.max(np.abs(wanth))
    assert not np.array_equal(gl[:, :6, :6], front.L_lidar[:, :6, :6])
    assert len(r.certs) == 4 and r.certs[-1].anchor_id == "depth_pose_evidence" and not r.certs[-1].exact
    row = lidar_cert_row([front.certs[1], visual_cert(front.vpe_cert, br2.config.eps_lift, br2.chart_id), r.certs[-1]],
                         [front.certs[0]])
    assert r.lidar_cert.tobytes() == row.tobytes() and gc.tobytes() == np.tile(row, (2, 1)).tobytes()
    assert np.all(np.isfinite(p1.get_beliefs()["L"]))


def test_step_refuses_more_than_32_hypotheses_with_a_frame(ctx):
    step, *_ , meas, s, MC = _step_setup(ctx)
    step.pipeline.Hl = 33  # the check reads the pipeline's hypothesis count before any device work
    try:
        with pytest.raises(ValueError, match="at most 32"):
            step.run(0, s, MC.SCAN_SEQ, MC.TIMESTAMP, measurement_batch=meas, depth_frame=_frame())
    finally:
        step.pipeline.Hl = 2
