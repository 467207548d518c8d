"""The batched pipeline with its LiDAR evidence given (GC_LIDAR_GIVEN: scan_front / set_lidar_evidence /
scan_back, csrc/gc_predio.hip and k_evidence_given) against the bin path's own bits for the front, and
against the given-evidence restatement (tests/primstep_restatement.py) for the rest, at the bars of
tests/test_gpu_pipeline.py:54-80. s_dt and s_ex have no bar there: they take beta's (1e-10 absolute:
scalars in [0, 1] formed from the same matrices); dPsi_proc takes Psi_proc's (1e-7 relative, 1e-18).

Shapes: cases.build(H=3, n_az=64) = 1,024 points (they feed only the budget scalars here); H = 3 covers
global hypothesis 0 and the others."""

import time

import numpy as np
import pytest

from oracle import gc_oracle as O
from oracle import cases
from test_gpu_pipeline import _close

import primstep_restatement as PR

pytestmark = pytest.mark.gpu

EPS_I = O.EPS_LIFT * np.eye(22)


def _pipe(case, ctx, given, io_computed=False, rank=0, world=1):
    from gcslam.pipeline import BatchedScanPipeline, PipelineConfig
    H = len(case["state"].beliefs)
    pipe = BatchedScanPipeline(H, case["n"], PipelineConfig(n_points_cap=case["n"]), rank=rank, world_size=world,
                               ctx=ctx)
    hy = case["hyp"]
    sl = slice(pipe.h0, pipe.h1)
    pipe.set_beliefs(hy["X_anchor"][sl], hy["z_lin"][sl], hy["L"][sl], hy["h"][sl], hy["stamp"][sl])
    pipe.set_weights(hy["weights"])
    if io_computed:
        pipe.set_io_mode(True)
    else:
        pipe.set_io_evidence(*(a[sl] for a in case["io"]))
    pipe.set_iw(*case["iw"])
    pipe.set_map(case["map_record"])
    if given:
        pipe.set_lidar_mode(True)
    return pipe


def _evidence(rng, H):
    """eps_lift I plus random SPD translation / rotation blocks (what visual_pose_evidence writes), a
    random pose part of h, and random certificate rows."""
    L, h = np.tile(EPS_I, (H, 1, 1)), np.zeros((H, 22))
    cert = np.empty((H, 6))
    for i in range(H):
        A, Bm = rng.normal(size=(3, 3)), rng.normal(size=(3, 3))
        L[i, 0:3, 0:3] += 30.0 * A @ A.T + 20.0 * np.eye(3)
        L[i, 3:6, 3:6] += 300.0 * Bm @ Bm.T + 100.0 * np.eye(3)
        h[i, 0:6] = rng.normal(size=6) * np.array([2.0, 2.0, 2.0, 5.0, 5.0, 5.0])
        cert[i] = [rng.uniform(5, 50), rng.uniform(0.3, 1.0), rng.uniform(0, 0.3), rng.uniform(0, 0.05),
                   rng.uniform(0, 0.05), rng.uniform(0, 1e-3)]
    return L, h, cert


def _given_scan(pipe, s, k, L, h, cert, slot=0):
    pipe.stage_scan(slot, s)
    pipe.scan_front(slot, s, k)
    pipe.set_lidar_evidence(L, h, cert)
    pipe.scan_back()


def _front_out(pipe):
    Lio, hio, cio = pipe.io_evidence()
    xi, ess = pipe.front_twists()
    return dict(io_L=Lio, io_h=hio, io_cert=cio, io_parts=pipe.io_parts(), xi=xi, ess_imu=ess,
                pose_pred=pipe.front_poses()[1])


def _same_bits(a, b, what):
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


# ------------------------------------------------------------------------------------- 1. front bits
@pytest.mark.parametrize("factorised", [False, True])
@pytest.mark.parametrize("io", ["synthetic", "computed"])
def test_front_is_the_bin_paths_bits(ctx, io, factorised):
    """scan_front against a bin-path pipeline's scan_local on the same state: the first scan from the
    uploaded beliefs, the second after one identical bin-path scan (the cached posterior factorisation,
    sig_cached, and with it the split predict: pred_mode 0), with the split or the factorised route."""
    case = cases.build(H=3, n_az=64, n_scans=2, io=io)
    comp = io == "computed"
    s0, s1 = case["scans"]
    A, Bp, G = _pipe(case, ctx, False, comp), _pipe(case, ctx, False, comp), _pipe(case, ctx, True, comp)
    for p in (A, Bp, G):
        p.set_predict_route(factorised)
    # ---- scan 1
    A.stage_scan(0, s0)
    A.run_scan_local(0, s0, 0)
    fa = _front_out(A)
    assert np.array_equal(fa["xi"], A.bin_stats()[2])
    G.stage_scan(0, s0)
    G.scan_front(0, s0, 0)
    _same_bits(fa, _front_out(G), "scan 1")
    G.set_lidar_evidence(np.tile(EPS_I, (3, 1, 1)), np.zeros((3, 22)), np.zeros(6))
    G.scan_back()
    G.finish_scan()
    A.finish_scan()
    assert A.hyp_conditioning()[:, 0].tobytes() == G.hyp_conditioning()[:, 0].tobytes()
    # ---- scan 2: a second bin-path pipeline repeats A's first scan, then takes the given-evidence front
    Bp.stage_scan(0, s0)
    Bp.run_scan(0, s0, 0)
    Bp.set_lidar_mode(True)
    A.stage_scan(0, s1)
    A.run_scan_local(0, s1, 1)
    Bp.stage_scan(0, s1)
    Bp.scan_front(0, s1, 1)
    _same_bits(_front_out(A), _front_out(Bp), "scan 2")
    assert A.hyp_conditioning()[:, 0].tobytes() == Bp.hyp_conditioning()[:, 0].tobytes()
    Bp.set_lidar_evidence(np.tile(EPS_I, (3, 1, 1)), np.zeros((3, 22)), np.zeros(6))
    Bp.scan_back()
    Bp.finish_scan()
    A.finish_scan()
    ctx.sync()


# ------------------------------------------------------------------------------ 2. linearisation pose
@pytest.mark.parametrize("io", ["synthetic", "computed"])
def test_linearisation_pose_matches_restatement(ctx, io):
    case = cases.build(H=3, n_az=64, n_scans=1, io=io)
    st, s = case["state"], case["scans"][0]
    G = _pipe(case, ctx, True, io == "computed")
    G.stage_scan(0, s)
    G.scan_front(0, s, 0)
    lin, pose_pred = G.front_poses()
    lin_d, pp_d = G.front_poses(device=True)
    assert lin_d.download().tobytes() == lin.tobytes() and pp_d.download().tobytes() == pose_pred.tobytes()
    Q = O.iw_process_Q(st.nu_proc, st.Psi_proc)
    Sga = (O.iw_meas_mode(st.nu_meas, st.Psi_meas, 0), O.iw_meas_mode(st.nu_meas, st.Psi_meas, 1))
    for i in range(3):
        f = PR.front(st.beliefs[i], cases.scan_input(s), Q, None if case["ios"] is None else case["ios"][i], Sga)
        _close(lin[i], PR.z_lin_pose(f["bpred"], f["io"]), 1e-6, 1e-9, f"hyp{i} z_lin_pose")
        _close(pose_pred[i], O.world_pose(f["bpred"]), 0.0, 1e-6, f"hyp{i} pose_pred")
    G.set_lidar_evidence(np.tile(EPS_I, (3, 1, 1)), np.zeros((3, 22)), np.zeros(6))
    G.scan_back()
    G.finish_scan()
    ctx.sync()


# ------------------------------------------------------------------------------------ 3. chain parity
def _compare_scan(pipe, res, comb, st, k, H):
    diag, bel, lpose = pipe.hyp_diag(), pipe.get_beliefs(), pipe.lpose6()
    dPsi = pipe.hyp_stats()[0]
    for i in range(H):
        r = res[i]
        _close(lpose[i], r["L_ev"][0:6, 0:6], 1e-8, 1e-10, f"scan{k} hyp{i} L_pose6")
        _close(diag[i, 13], r["cond6"], 1e-6, 0, f"scan{k} hyp{i} cond_pose6")
        _close(diag[i, 39], r["eigmin6"], 1e-7, 1e-12, f"scan{k} hyp{i} eigmin_pose6")
        _close(diag[i, 30:36], r["xi_body"], 1e-9, 1e-12, f"scan{k} hyp{i} xi_body")
        assert abs(diag[i, 6] - r["T"]) <= 1e-8 * abs(r["T"]) + 1e-10, (k, i, diag[i, 6], r["T"])
        assert abs(diag[i, 7] - r["beta"]) < 1e-10 and abs(diag[i, 8] - r["alpha"]) < 1e-12
        assert abs(diag[i, 9] - r["s_dt"]) < 1e-10 and abs(diag[i, 10] - r["s_ex"]) < 1e-10
        assert abs(diag[i, 11] - r["rho"]) < 1e-8
        assert not diag[i, 18:20].any() and not diag[i, 21:30].any()
        b = r["belief"]
        _close(diag[i, 0:6], r["pose"], 0.0, 1e-6, f"scan{k} hyp{i} world pose")
        _close(bel["X_anchor"][i], b.X_anchor, 0.0, 1e-6, f"scan{k} hyp{i} X_anchor")
        _close(bel["L"][i], b.L, 1e-8, 0.0, f"scan{k} hyp{i} L")
        _close(bel["z_lin"][i], b.z_lin, 1e-6, 1e-9, f"scan{k} hyp{i} z_lin")
        _close(dPsi[i], r["dPsi_proc"], 1e-7, 1e-18, f"scan{k} hyp{i} dPsi_proc")
    c = pipe.combined()
    _close(c["L"], comb["L"], 1e-8, 0.0, f"scan{k} combined L")
    _close(c["h"], comb["h"], 1e-6, 1e-9, f"scan{k} combined h")
    _close(c["z_lin"], comb["z_lin"], 1e-6, 1e-9, f"scan{k} combined z_lin")
    iw = pipe.get_iw()
    _close(iw["nu_proc"], st.nu_proc, 1e-12, 0, "nu_proc")
    _close(iw["Psi_proc"], st.Psi_proc, 1e-7, 1e-18, "Psi_proc")
    _close(iw["Psi_meas"], st.Psi_meas, 1e-7, 1e-18, "Psi_meas")
    _close(iw["Q"], O.iw_process_Q(st.nu_proc, st.Psi_proc), 1e-7, 1e-18, "Q")


@pytest.mark.parametrize("rows", ["one", "per_hypothesis"])
def test_chain_matches_restatement_over_scans(ctx, rows):
    H = 3
    case = cases.build(H=H, n_az=64, n_scans=3)
    pipe = _pipe(case, ctx, True)
    map0 = pipe.get_map()
    rng = np.random.default_rng(7)
    st = case["state"]
    for k, s in enumerate(case["scans"]):
        L, h, cert = _evidence(rng, H)
        cert = cert[0] if rows == "one" else cert
        _given_scan(pipe, s, st.scan_count, L, h, cert)
        pipe.finish_scan()
        st, comb, res = PR.process_scan_given(st, cases.scan_input(s), case["ios"], L, h, cert)
        ctx.sync()
        gl, gh, gc = pipe.lidar_evidence()
        assert gl.tobytes() == L.tobytes() and gh.tobytes() == h.tobytes()
        assert gc.tobytes() == np.ascontiguousarray(np.broadcast_to(cert, (H, 6))).tobytes()
        _compare_scan(pipe, res, comb, st, k, H)
        # hypothesis 0's z_t record, without a scan map attached
        z_t, Sig_pose, xi0 = pipe.scan_map_pose()
        _close(z_t, res[0]["z_t"], 0.0, 1e-6, f"scan{k} z_t")
        _close(xi0, res[0]["xi_body"], 1e-9, 1e-12, f"scan{k} xi_body of the record")
    map1 = pipe.get_map()
    for key in ("map", "derived"):
        assert map0[key].tobytes() == map1[key].tobytes(), key
    assert (map0["z_scale"], map0["N_dir_total"]) == (map1["z_scale"], map1["N_dir_total"])


# ------------------------------------------------------------------------------------------ 4. edges
def test_edge_no_map_branch_takes_the_certified_fusion(ctx):
    """L_lidar = eps_lift I, h = 0 (pipeline.py:1014-1015): the chain with the IMU/odom evidence alone; the
    fusion's projection is certified (delta exactly 0)."""
    H = 3
    case = cases.build(H=H, n_az=64, n_scans=1)
    L, h = PR.eps_lift_evidence(H)
    cert = np.zeros(6)
    st, s = case["state"], case["scans"][0]
    with O.exact_inactive_deltas():
        _, _, res0 = PR.process_scan_given(st, cases.scan_input(s), case["ios"], L, h, cert)
    assert all(r["fc"][0] == 0.0 for r in res0)  # the chosen input takes the certified route
    pipe = _pipe(case, ctx, True)
    _given_scan(pipe, s, st.scan_count, L, h, cert)
    pipe.finish_scan()
    st1, comb, res = PR.process_scan_given(st, cases.scan_input(s), case["ios"], L, h, cert)
    ctx.sync()
    _compare_scan(pipe, res, comb, st1, 0, H)
    assert np.all(pipe.hyp_diag()[:, 20] == 0.0)


def test_edge_indefinite_posterior_takes_the_projection(ctx):
    """An evidence whose pose block is negative enough that L_post is indefinite: the fusion runs the
    Jacobi projection (wg_psd_fast_lifted_chol) and reports its delta."""
    H = 3
    case = cases.build(H=H, n_az=64, n_scans=1)
    L, h = PR.eps_lift_evidence(H)
    L[:, 0:6, 0:6] -= 1e8 * np.eye(6)
    cert = np.array([10.0, 0.8, 0.05, 0.0, 0.0, 1e-4])
    st, s = case["state"], case["scans"][0]
    with O.exact_inactive_deltas():
        _, _, res0 = PR.process_scan_given(st, cases.scan_input(s), case["ios"], L, h, cert)
    assert all(r["fc"][0] > 0.0 for r in res0)  # the chosen input takes the projected route
    pipe = _pipe(case, ctx, True)
    _given_scan(pipe, s, st.scan_count, L, h, cert)
    pipe.finish_scan()
    ctx.sync()
    diag = pipe.hyp_diag()
    assert np.all(diag[:, 20] > 0.0), diag[:, 20]
    for i in range(H):
        _close(diag[i, 20], res0[i]["fc"][0], 1e-6, 0.0, f"hyp{i} fusion psd delta")
    assert np.all(np.isfinite(pipe.get_beliefs()["L"]))


# ----------------------------------------------------------------------------------------- 5. shards
def test_shards_match_unsharded_bit_for_bit(ctx):
    """H = 4 as 2 + 2 on one GPU through get_partial / finish_scan(gathered), two scans."""
    H = 4
    case = cases.build(H=H, n_az=64, n_scans=2)
    full = _pipe(case, ctx, True)
    shards = [_pipe(case, ctx, True, rank=r, world=2) for r in range(2)]
    rng = np.random.default_rng(11)
    for k, s in enumerate(case["scans"]):
        L, h, cert = _evidence(rng, H)
        _given_scan(full, s, k, L, h, cert)
        full.finish_scan()
        for p in shards:
            sl = slice(p.h0, p.h1)
            _given_scan(p, s, k, L[sl], h[sl], cert[sl])
        recs = np.stack([p.partial() for p in shards])
        for p in shards:
            p.finish_scan(recs)
        ctx.sync()
        fb = full.get_beliefs()
        for name, get in (("diag", lambda p: p.hyp_diag()), ("lpose", lambda p: p.lpose6()),
                          ("dPsi_proc", lambda p: p.hyp_stats()[0]), ("Sigma", lambda p: p.hyp_stats()[2]),
                          ("lin_pose", lambda p: p.front_poses()[0])):
            cat = np.concatenate([get(p) for p in shards])
            assert cat.tobytes() == get(full).tobytes(), (k, name)
        for f in fb:
            cat = np.concatenate([p.get_beliefs()[f] for p in shards])
            assert cat.tobytes() == fb[f].tobytes(), (k, f)
        cf = full.combined()
        for p in shards:
            c = p.combined()
            for f in ("L", "h", "z_lin", "X_anchor"):
                assert c[f].tobytes() == cf[f].tobytes(), (k, p.rank, f)
            iw, iwf = p.get_iw(), full.get_iw()
            for f in ("nu_proc", "Psi_proc", "nu_meas", "Psi_meas", "Q"):
                assert iw[f].tobytes() == iwf[f].tobytes(), (k, p.rank, f)


# ------------------------------------------------------------------------------------ 6. state rules
def test_state_rules(ctx):
    from gcslam.primitive_map import DevicePrimitiveMap
    H = 3
    case = cases.build(H=H, n_az=64, n_scans=1)
    s = case["scans"][0]
    L, h = PR.eps_lift_evidence(H)
    cert = np.zeros(6)
    dm = DevicePrimitiveMap(1, 64, ctx=ctx)
    # ---- bin mode: no front, no evidence, no back
    p = _pipe(case, ctx, False)
    p.stage_scan(0, s)
    with pytest.raises(ValueError, match="GC_LIDAR_GIVEN"):
        p.scan_front(0, s, 0)
    with pytest.raises(ValueError, match="between gc_pipeline_scan_front and gc_pipeline_scan_back"):
        p.set_lidar_evidence(L, h, cert)
    with pytest.raises(ValueError, match="no front"):
        p.scan_back()
    # ---- a scan map and the given mode exclude each other
    p.attach_primitive_map(dm)
    with pytest.raises(ValueError, match="scan map is attached"):
        p.set_lidar_mode(True)
    p.attach_primitive_map(None)
    p.set_lidar_mode(True)
    with pytest.raises(ValueError, match="takes no scan map"):
        p.attach_primitive_map(dm)
    with pytest.raises(ValueError, match="lidar mode must be"):
        p._call("gc_pipeline_set_lidar_mode", 2)
    # ---- given mode: the bin path's entries are refused
    with pytest.raises(ValueError, match="gc_pipeline_scan_front"):
        p.run_scan_local(0, s, 0)
    with pytest.raises(ValueError, match="gc_pipeline_scan_front"):
        p.run_scan(0, s, 0)
    with pytest.raises(ValueError, match="no bin statistics"):
        p.bin_stats()
    with pytest.raises(ValueError, match="no bin, MF or planar"):
        p.projection_certs()
    with pytest.raises(ValueError, match="no front"):
        p.scan_back()
    # ---- front .. back
    p.scan_front(0, s, 0)
    with pytest.raises(ValueError, match="already enqueued"):
        p.scan_front(0, s, 0)
    with pytest.raises(ValueError, match="not set"):
        p.scan_back()
    with pytest.raises(ValueError, match="pending"):
        p.set_lidar_mode(False)
    with pytest.raises(ValueError, match="pending"):
        p.set_weights(case["hyp"]["weights"])
    with pytest.raises(ValueError, match="cert_rows"):
        p.set_lidar_evidence(L, h, np.zeros((2, 6)))
    p.set_lidar_evidence(L, h, cert)
    p.scan_back()
    with pytest.raises(ValueError, match="between gc_pipeline_scan_front and gc_pipeline_scan_back"):
        p.set_lidar_evidence(L, h, cert)
    with pytest.raises(ValueError, match="pending"):
        p.scan_front(0, s, 1)
    with pytest.raises(ValueError, match="pending"):
        p.set_lidar_mode(False)
    assert p.partial().shape[0] > 0
    p.finish_scan()
    p.set_lidar_mode(False)  # between scans the mode may change
    p.stage_scan(0, s)
    p.run_scan(0, s, 1)
    ctx.sync()


def test_restaging_the_fronts_slot_does_not_wait(ctx):
    """The front is the slot's last reader and releases it itself: behind a 0.5 s device spin, staging
    the next scan into the same slot after scan_front returns at once, and the scan staged second does
    not disturb the first (its results are those of an undisturbed run)."""
    from gcslam import _abi
    H = 3
    case = cases.build(H=H, n_az=64, n_scans=2)
    s0, s1 = case["scans"]
    L, h = PR.eps_lift_evidence(H)
    ref = _pipe(case, ctx, True)
    _given_scan(ref, s0, 0, L, h, np.zeros(6))
    ref.finish_scan()
    want = ref.get_beliefs()
    p = _pipe(case, ctx, True)
    p.stage_scan(0, s0)
    ctx.sync()
    _abi.call("gc_test_device_spin", ctx.handle, 0.5, ctx=ctx)
    t0 = time.perf_counter()
    p.scan_front(0, s0, 0)
    p.stage_scan(0, s1)
    t1 = time.perf_counter()
    print(f"front + restage {t1 - t0:.5f} s")
    assert t1 - t0 < 0.25, t1 - t0
    p.set_lidar_evidence(L, h, np.zeros(6))
    p.scan_back()
    p.finish_scan()
    got = p.get_beliefs()
    for f in want:
        assert got[f].tobytes() == want[f].tobytes(), f
    # and the restaged slot holds the second scan
    p.scan_front(0, s1, 1)
    ref.stage_scan(0, s1)
    ref.scan_front(0, s1, 1)
    assert p.front_poses()[0].tobytes() == ref.front_poses()[0].tobytes()
    for q in (p, ref):
        q.set_lidar_evidence(L, h, np.zeros(6))
        q.scan_back()
        q.finish_scan()
    ctx.sync()


# ------------------------------------------------- the map branch's evidence, handed over on the device
def test_map_branch_evidence_stays_on_the_device(ctx):
    """MapBranch.front with the poses as a DeviceArray and device_out=True on the `ragged` map-update
    geometry: the same bits as the default call on a second map, with L_lidar / h_lidar left in HBM; a
    pipeline takes them in place (set_lidar_evidence copies device to device on the stream) and runs its
    back on them: the result is that of the same evidence uploaded from the host."""
    from gcslam import _abi
    from gcslam.map_branch import MapBranch
    from gcslam.primitive_step import lidar_cert_row, visual_cert
    from test_gpu_mapbranch import _branch_config
    from test_gpu_mapupdate import _Obj, _fresh_map
    import mapupdate_cases as MC
    mcase = MC.build("ragged")
    cfg = _branch_config(mcase["m_view"], mcase["K"], mcase["k_ins"])
    meas = _Obj(**mcase["meas"])
    center = np.array([1.0, 0.5, 1.0])
    poses = np.stack([mcase["pose"], mcase["pose"] + np.array([0.05, -0.02, 0.01, 0.01, -0.02, 0.03])])
    f_host = MapBranch(_fresh_map(ctx, mcase), cfg).front(meas, center, poses, MC.SCAN_SEQ)
    d_poses = _abi.DeviceArray.from_host(ctx, poses)
    f_dev = MapBranch(_fresh_map(ctx, mcase), cfg).front(meas, center, d_poses, MC.SCAN_SEQ, device_out=True)
    assert f_host.device is None and isinstance(f_dev.L_lidar, _abi.DeviceArray)
    assert f_dev.device["L_lidar"] is f_dev.L_lidar and f_dev.device["h_lidar"] is f_dev.h_lidar
    assert np.asarray(f_dev.L_lidar).tobytes() == f_host.L_lidar.tobytes()
    assert np.asarray(f_dev.h_lidar).tobytes() == f_host.h_lidar.tobytes()
    assert f_dev.vpe_parts.tobytes() == f_host.vpe_parts.tobytes() and f_dev.vpe_cert.tobytes() == f_host.vpe_cert.tobytes()
    assert not np.array_equal(f_host.h_lidar[0, 0:6], f_host.h_lidar[1, 0:6])  # the two poses' evidence differs
    # ---- into a pipeline of two hypotheses
    H = 2
    case = cases.build(H=H, n_az=64, n_scans=1)
    s = case["scans"][0]
    row = lidar_cert_row([f_dev.certs[1], visual_cert(f_dev.vpe_cert, cfg.eps_lift)], [f_dev.certs[0]])
    outs = []
    for L, h in ((f_dev.device["L_lidar"], f_dev.device["h_lidar"]), (f_host.L_lidar, f_host.h_lidar)):
        pipe = _pipe(case, ctx, True)
        _given_scan(pipe, s, 0, L, h, row)
        pipe.finish_scan()
        gl, gh, gc = pipe.lidar_evidence()
        assert gl.tobytes() == f_host.L_lidar.tobytes() and gh.tobytes() == f_host.h_lidar.tobytes()
        assert gc.tobytes() == np.tile(row, (H, 1)).tobytes()
        b = pipe.get_beliefs()
        outs.append((b["L"], b["h"], b["z_lin"], b["X_anchor"], pipe.hyp_diag(), pipe.combined()["L"]))
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    st1, comb, res = PR.process_scan_given(case["state"], cases.scan_input(s), case["ios"], f_host.L_lidar,
                                           f_host.h_lidar, row)
    _compare_scan(pipe, res, comb, st1, 0, H)


# ------------------------------------------------------------------------------------- 7. the step
SHIFT = np.array([0.3, 0.2, 0.5])  # the hypotheses' anchors well inside hex cell (0, 0, 0) of the `ragged` map


def _step_case(n_scans):
    """cases.build(H=2) with the anchors moved by SHIFT (device and oracle alike) and the scan counter at the
    map case's scan_seq (the step passes one counter to the pipeline and to the map branch)."""
    import dataclasses
    import mapupdate_cases as MC
    case = cases.build(H=2, n_az=64, n_scans=n_scans)
    hy = dict(case["hyp"])
    hy["X_anchor"] = hy["X_anchor"].copy()
    hy["X_anchor"][:, 0:3] += SHIFT
    beliefs = [O.Belief(hy["X_anchor"][i].copy(), b.z_lin.copy(), b.L.copy(), b.h.copy())
               for i, b in enumerate(case["state"].beliefs)]
    return dict(case, hyp=hy, state=dataclasses.replace(case["state"], beliefs=beliefs, scan_count=MC.SCAN_SEQ))


def _by_hand(pipe, branch, s, seq, timestamp, meas=None, surfel_config=None):
    """PrimitiveScanStep.run's calls made one by one through the public entries."""
    from gcslam.ops.deskew_constant_twist import deskew_constant_twist
    from gcslam.ops.lidar_surfel_extraction import extract_lidar_surfels
    from gcslam.ops.point_budget import point_budget_resample
    from gcslam.primitive_step import lidar_cert_row, visual_cert
    ctx = pipe.ctx
    pipe.stage_scan(0, s)
    pipe.scan_front(0, s, seq)
    xi, ess = pipe.front_twists()
    centre = pipe.front_poses()[1][0, 0:3]
    lin_d = pipe.front_poses(device=True)[0]
    bcerts = []
    if meas is None:
        bud, _, _ = point_budget_resample(s["points"], s["timestamps"], s["weights"], n_points_cap=pipe.cfg.n_points_cap,
                                          chart_id=branch.chart_id, ctx=ctx, device_out=True)
        dsk, dc, _ = deskew_constant_twist(bud.points, bud.timestamps, bud.weights, float(s["scan_start"]),
                                           float(s["scan_end"]), xi[0], float(ess[0]), branch.chart_id,
                                           "deskew_constant_twist", ctx=ctx, device_out=True)
        meas, sc, _ = extract_lidar_surfels(dsk.points, dsk.timestamps, dsk.weights, surfel_config,
                                            chart_id=branch.chart_id, ctx=ctx, device_out=True)
        bcerts = [dc, sc]
    front = branch.front(meas, centre, lin_d, seq, device_out=True)
    row = lidar_cert_row(bcerts + [front.certs[1], visual_cert(front.vpe_cert, branch.config.eps_lift, branch.chart_id)],
                         [front.certs[0]])
    pipe.set_lidar_evidence(front.device["L_lidar"], front.device["h_lidar"], row)
    pipe.scan_back()
    pipe.finish_scan()
    z_t = pipe.scan_map_pose()[0]
    return front, row, branch.update(front, z_t, timestamp), z_t


def _same_step(r, hand, p1, p2, dm1, dm2):
    from test_gpu_mapbranch import _bits, _same_update
    front2, row2, upd2, z_t2 = hand
    assert np.asarray(r.front.L_lidar).tobytes() == np.asarray(front2.L_lidar).tobytes()
    assert np.asarray(r.front.h_lidar).tobytes() == np.asarray(front2.h_lidar).tobytes()
    assert r.lidar_cert.tobytes() == row2.tobytes() and r.z_t.tobytes() == z_t2.tobytes()
    b1, b2 = p1.get_beliefs(), p2.get_beliefs()
    for f in b1:
        assert b1[f].tobytes() == b2[f].tobytes(), f
    c2 = p2.combined()
    for f in ("L", "h", "z_lin", "X_anchor"):
        assert r.combined[f].tobytes() == c2[f].tobytes(), f
    _same_update(r.update, upd2)
    assert _bits(dm1.download()) == _bits(dm2.download())
    assert (dm1.next_global_id, dm1.total_count, dm1.tile_count) == (dm2.next_global_id, dm2.total_count, dm2.tile_count)


def test_step_three_scans_supplied_batch(ctx):
    """PrimitiveScanStep.run on the `ragged` map-update geometry, H = 2, three scans with a caller-supplied
    batch: the same bits as the same calls made by hand on a second map and pipeline, and the restatement
    fed tests/vpe_restatement.py's evidence at the oracle's association of the map as it stood before each
    scan, at the bars of tests/test_gpu_visual_pose.py (evidence) and of the chain test above."""
    from gcslam.map_branch import MapBranch
    from gcslam.primitive_step import PrimitiveScanStep
    from test_association import _cmp
    from test_gpu_mapbranch import _branch_config
    from test_gpu_mapupdate import _Obj, _fresh_map, _tiles_of
    import mapupdate_cases as MC
    import vpe_cases as VC
    import vpe_restatement as VR
    H = 2
    mcase = MC.build("ragged")
    cfg = _branch_config(mcase["m_view"], mcase["K"], mcase["k_ins"])
    meas = _Obj(**mcase["meas"])
    case = _step_case(3)
    dm1, dm2 = _fresh_map(ctx, mcase), _fresh_map(ctx, mcase)
    p1, p2 = _pipe(case, ctx, False), _pipe(case, ctx, True)
    step, br2 = PrimitiveScanStep(p1, MapBranch(dm1, cfg)), MapBranch(dm2, cfg)
    st = case["state"]
    inserted = 0
    for k, s in enumerate(case["scans"]):
        seq, ts = MC.SCAN_SEQ + k, MC.TIMESTAMP + 0.1 * k
        tiles = _tiles_of(dm2)  # the map before the scan: the oracle's input
        r = step.run(0, s, seq, ts, measurement_batch=meas)
        _same_step(r, _by_hand(p2, br2, s, seq, ts, meas=meas), p1, p2, dm1, dm2)
        # ---- conditions
        assert r.front.active_tile_ids == mcase["active"], k
        assert r.update[0].n_fused > 0, k
        inserted += r.update[0].n_inserted
        L_gpu, h_gpu = np.asarray(r.front.L_lidar), np.asarray(r.front.h_lidar)
        assert not np.array_equal(h_gpu[0, 0:6], h_gpu[1, 0:6]), k
        # ---- the oracle's branch on the map as it stood: recency inflate, view, association, evidence
        for a in r.front.active_tile_ids:
            if a in tiles:
                tiles[a] = O.primitive_map_recency_inflate(tiles[a], seq, cfg.RECENCY_DECAY_LAMBDA,
                                                           cfg.RECENCY_MIN_SCALE)[0]
        view = O.extract_atlas_map_view(tiles, r.front.stencil_tile_ids, cfg.M_TILE_VIEW, mcase["m_tile"])
        ores, _ = O.associate_primitives_ot(mcase["meas"], view, dict(k_assoc=mcase["K"], scan_seq=seq, h_tile=MC.H_TILE))
        lin_gpu = p1.front_poses()[0]
        at_gpu = [VR.visual_pose_evidence(ores, mcase["meas"], view, lin_gpu[i]) for i in range(H)]
        VC.check_conditions(at_gpu)
        for i in range(H):
            _cmp(dict(L_pose=L_gpu[i], h_pose=h_gpu[i]), {f: at_gpu[i][f] for f in ("L_pose", "h_pose")}, (), 1e-10)
        # ---- the chain on the restatement's own linearisation poses and evidence
        Q = O.iw_process_Q(st.nu_proc, st.Psi_proc)
        zl = [PR.z_lin_pose(f["bpred"], f["io"]) for f in
              (PR.front(st.beliefs[i], cases.scan_input(s), Q, case["ios"][i]) for i in range(H))]
        ref = [VR.visual_pose_evidence(ores, mcase["meas"], view, zl[i]) for i in range(H)]
        for i in range(H):
            _close(lin_gpu[i], zl[i], 1e-6, 1e-9, f"scan{k} hyp{i} z_lin_pose")
        st, comb, res = PR.process_scan_given(st, cases.scan_input(s), case["ios"], np.stack([x["L_pose"] for x in ref]),
                                              np.stack([x["h_pose"] for x in ref]), r.lidar_cert)
        _compare_scan(p1, res, comb, st, k, H)
        _close(r.z_t, res[0]["z_t"], 0.0, 1e-6, f"scan{k} z_t")
    assert inserted > 0


def test_step_builds_the_batch_from_the_scan(ctx):
    """No batch given: the step budgets the 1,024-point scan, deskews it with hypothesis 0's twist and
    extracts surfels on the device. The config is small enough for >= 8 valid surfels (checked on the CPU
    with tests/surfel_restatement.py on the oracle's deskewed points); the run equals the calls by hand."""
    from gcslam.map_branch import MapBranch
    from gcslam.ops.lidar_surfel_extraction import SurfelExtractionConfig
    from gcslam.primitive_step import PrimitiveScanStep
    from test_gpu_mapbranch import _branch_config
    from test_gpu_mapupdate import _fresh_map
    import mapupdate_cases as MC
    import surfel_restatement as SR
    sdict = dict(n_surfel=64, n_feat=4, voxel_size_m=1.0, min_points_per_voxel=5, hex3d_num_cells_1=8,
                 hex3d_num_cells_2=8, hex3d_num_cells_z=4, hex3d_max_occupants=32)
    mcase = MC.build("ragged")
    cfg = _branch_config(mcase["m_view"], mcase["K"], mcase["k_ins"])
    case = _step_case(1)
    s, st = case["scans"][0], case["state"]
    # ---- on the CPU: the oracle's twist of hypothesis 0, its deskew, the restatement's surfels
    scan = cases.scan_input(s)
    f0 = PR.front(st.beliefs[0], scan, O.iw_process_Q(st.nu_proc, st.Psi_proc), case["ios"][0])
    bud = O.point_budget_resample(scan.points, scan.timestamps, scan.weights, scan.ring, scan.tag, case["n"])
    p0, wd, _ = O.deskew_constant_twist(bud["points"], bud["timestamps"], bud["weights"], scan.scan_start,
                                        scan.scan_end, f0["xi"])
    n_cpu = int(SR.extract(p0, bud["timestamps"], wd, sdict)["valid_mask"].sum())
    assert n_cpu >= 8, n_cpu
    # ---- the step against the calls by hand
    scfg = SurfelExtractionConfig(**sdict)
    dm1, dm2 = _fresh_map(ctx, mcase), _fresh_map(ctx, mcase)
    p1, p2 = _pipe(case, ctx, False), _pipe(case, ctx, True)
    step = PrimitiveScanStep(p1, MapBranch(dm1, cfg), scfg)
    r = step.run(0, s, MC.SCAN_SEQ, MC.TIMESTAMP)
    _same_step(r, _by_hand(p2, MapBranch(dm2, cfg), s, MC.SCAN_SEQ, MC.TIMESTAMP, surfel_config=scfg), p1, p2, dm1, dm2)
    nv = int(r.front.measurement_batch.n_lidar_valid)
    print(f"valid surfels: device {nv}, restatement {n_cpu}")
    assert nv >= 8
    assert len(r.certs) == 5 and r.certs[1].support.ess_total == float(nv)
    _close(r.xi_body, f0["xi"], 1e-9, 1e-12, "xi_body")
    assert np.all(np.isfinite(p1.get_beliefs()["L"]))


def test_step_is_single_rank(ctx):
    from gcslam.map_branch import MapBranch
    from gcslam.primitive_map import DevicePrimitiveMap
    from gcslam.primitive_step import PrimitiveScanStep
    case = cases.build(H=2, n_az=64, n_scans=1)
    with pytest.raises(ValueError, match="single rank"):
        PrimitiveScanStep(_pipe(case, ctx, False, rank=0, world=2), MapBranch(DevicePrimitiveMap(9, 64, ctx=ctx)))
