"""CPU checks of the primitive-map scan step's host side: the given-evidence restatement
(tests/primstep_restatement.py) pinned to the pinned oracle, the certificate row the step hands to the
device, and the bindings of the GC_LIDAR_GIVEN entries."""

import numpy as np

from oracle import gc_oracle as O
from oracle import cases

import primstep_restatement as PR


def _bin_side(r, pre_ess):
    """What O.scan_hypothesis's bin path feeds its evidence sum, as a given LiDAR evidence: the MF + planar
    blocks and the aggregate of [deskew, assign, moments, MF, planar] (gc_oracle.py:1304-1315, :1322)."""
    L, h = np.zeros((O.D_Z, O.D_Z)), np.zeros(O.D_Z)
    tr, mf, sa, mm = r["planar"], r["mf"], r["assign"], r["moments"]
    L[0:3, 0:3] = tr["L_trans"]; h[0:3] = tr["h_trans"]
    L[3:6, 3:6] = mf["L_rot"]; h[3:6] = mf["h_rot"]
    ess_ev = (pre_ess + sa["ess"] + mm["ess"] + 0.0 + 0.0) / 5.0
    sf_ev = (r["retained"] + sa["max_resp"] + mm["support_frac"] + 1.0 + 1.0) / 5.0
    cert = [ess_ev, sf_ev, mf["nll_per_ess"] + tr["nll_per_ess"], 0.0, 0.0,
            [sa["trig"], mm["trig"], mf["trig"], tr["trig"]]]
    return L, h, cert


def test_restatement_is_the_oracle_with_the_bin_evidence_given():
    """Fed the bin path's own evidence and certificate values, the given-evidence restatement is
    O.scan_hypothesis's arithmetic: every shared output is EQUAL."""
    case = cases.build(H=3, n_az=64, n_scans=2)
    st = case["state"]
    for k, s in enumerate(case["scans"]):
        scan = cases.scan_input(s)
        Q = O.iw_process_Q(st.nu_proc, st.Psi_proc)
        st_next, _, res = O.process_scan(st, scan, case["ios"], case["bins"], case["cfg"])
        for i, r in enumerate(res):
            pre_ess = PR.front(st.beliefs[i], scan, Q, case["ios"][i])["pre"]["ess"]
            L, h, cert = _bin_side(r, pre_ess)
            g = PR.scan_hypothesis_given(st.beliefs[i], scan, Q, case["ios"][i], L, h, cert)
            for key in ("T", "beta", "alpha", "s_dt", "s_ex", "rho"):
                assert g[key] == r[key], (k, i, key, g[key], r[key])
            assert np.array_equal(g["dPsi_proc"], r["dPsi_proc"]), (k, i)
            for f in ("X_anchor", "z_lin", "L", "h"):
                assert np.array_equal(getattr(g["belief"], f), getattr(r["belief"], f)), (k, i, f)
            assert np.array_equal(g["xi_body"], r["xi_body"]) and np.array_equal(g["L_ev"], r["L_ev"])
        st = st_next


def test_restatement_linearisation_pose_and_empty_branch():
    case = cases.build(H=3, n_az=64, n_scans=1)
    st, scan = case["state"], cases.scan_input(case["scans"][0])
    Q = O.iw_process_Q(st.nu_proc, st.Psi_proc)
    L0, h0 = PR.eps_lift_evidence()
    assert np.array_equal(L0, O.EPS_LIFT * np.eye(22)) and not h0.any()
    g = PR.scan_hypothesis_given(st.beliefs[1], scan, Q, case["ios"][1], L0, h0, np.zeros(6))
    bpred = O.predict_diffusion(st.beliefs[1], Q, scan.dt_sec)[0]
    io = case["ios"][1]
    z = np.linalg.solve(O.psd_project(bpred.L + io.L)[0] + O.EPS_LIFT * np.eye(22), bpred.h + io.h)
    assert np.allclose(g["z_lin_pose"], z[:6], rtol=1e-9, atol=1e-12)
    # the fusion's clamp is inactive on this input: with the eigen-round-off of an inactive projection
    # reported as 0 (O.exact_inactive_deltas), its delta is exactly 0
    with O.exact_inactive_deltas():
        g0 = PR.scan_hypothesis_given(st.beliefs[1], scan, Q, case["ios"][1], L0, h0, np.zeros(6))
    assert g0["fc"][0] == 0.0 and g["fc"][0] < 1e-9


def test_lidar_cert_row_by_hand():
    from gcslam.certificates import (CertBundle, ExcitationCert, InfluenceCert, MismatchCert, SupportCert)
    from gcslam.primitive_step import lidar_cert_row, visual_cert
    mk = lambda ess, sf, nll, edt, eex, **inf: CertBundle.create_approx(  # noqa: E731
        chart_id="c", anchor_id="a", triggers=["t"], support=SupportCert(ess_total=ess, support_frac=sf),
        mismatch=MismatchCert(nll_per_ess=nll), excitation=ExcitationCert(dt_effect=edt, extrinsic_effect=eex),
        influence=InfluenceCert.identity().with_overrides(**inf))
    deskew = mk(37.5, 0.93, 0.0, 0.0, 0.0)
    surfel = mk(12.0, 0.75, 0.0, 0.01, 0.0)
    assoc = mk(9.25, 0.5, 0.125, 0.0, 0.03, mass_epsilon_ratio=2e-3, psd_projection_delta=1e-4)
    visual = mk(8.0, 1.0, 0.25, 0.0, 0.02, lift_strength=1e-9)
    inflate = mk(0.0, 1.0, 0.0, 0.0, 0.0, dt_scale=0.75)
    row = lidar_cert_row([deskew, surfel, assoc, visual], [inflate])
    assert row.shape == (6,)
    assert row[0] == (37.5 + 12.0 + 9.25 + 8.0) / 4.0 and row[1] == (0.93 + 0.75 + 0.5 + 1.0) / 4.0
    assert row[2] == 0.0 + 0.0 + 0.125 + 0.25
    assert row[3] == 0.01 and row[4] == 0.03
    trig = 0.0 + 0.0 + O.trigger(mass=2e-3, psd=1e-4) + O.trigger(lift=1e-9) + O.trigger(dt=0.75)
    assert abs(row[5] - trig) <= 1e-15
    # only the evidence certificates are aggregated: the extra one adds to the trigger sum alone
    row2 = lidar_cert_row([deskew, surfel, assoc, visual])
    assert np.array_equal(row2[:5], row[:5]) and abs(row[5] - row2[5] - 0.25) <= 1e-15
    # visual_pose_evidence's certificate from the batched operator's cert_vec
    v = visual_cert(np.array([5.0, 7.0, 3.5, 0.7]), 1e-9)
    assert (v.support.ess_total, v.support.support_frac, v.influence.lift_strength, v.exact) == (3.5, 1.0, 1e-9, False)
    assert visual_cert(np.array([0.0, 7.0, 0.0, 0.0]), 1e-9).exact


def test_bindings_cover_the_given_mode():
    from gcslam import _abi
    names = ("gc_pipeline_set_lidar_mode", "gc_pipeline_scan_front", "gc_pipeline_front_poses",
             "gc_pipeline_get_front_poses", "gc_pipeline_get_front_twists", "gc_pipeline_get_front_hyp0",
             "gc_pipeline_set_lidar_evidence", "gc_pipeline_get_lidar_evidence", "gc_pipeline_scan_back")
    assert all(n in _abi.SIGNATURES for n in names)
    assert (_abi.GC_LIDAR_BINS, _abi.GC_LIDAR_GIVEN, _abi.GC_LIDAR_CERT) == (0, 1, 6)
    from gcslam.pipeline import BatchedScanPipeline
    for m in ("set_lidar_mode", "scan_front", "front_poses", "set_lidar_evidence", "scan_back", "lidar_evidence"):
        assert callable(getattr(BatchedScanPipeline, m))
    from gcslam.primitive_step import PrimitiveScanStep
    assert callable(PrimitiveScanStep.run)
