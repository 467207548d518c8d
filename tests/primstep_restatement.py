"""TEST INFRASTRUCTURE — the reference's current scan step (backend/pipeline.py:595-776 for the
IMU/odom side and the linearisation pose, :1038-1230 from the evidence sum on) restated for one
hypothesis with the LiDAR evidence GIVEN: the primitive-map branch's L_lidar / h_lidar (:998-1015)
and its aggregated certificate. Composed only of oracle.gc_oracle functions, in the reference's order;
it is O.scan_hypothesis with the bin path (a4-a8, the bin map's increment) taken out and the
certificate aggregation of :1056-1067 in place of the bin path's.

lidar_cert = [ess_total, support_frac, nll_per_ess, exc_dt, exc_ex, trigger] of
aggregate_certificates([deskew, surfel, assoc, visual]); its last entry is the LiDAR-side operators'
trigger magnitude: a scalar (their sum, as the device row carries it), or a sequence of per-operator
magnitudes, added one by one in order as the reference's sum over all_certs does (:1211)."""

from __future__ import annotations

import math

import numpy as np

from oracle import gc_oracle as O


def z_lin_pose(bpred: O.Belief, io: O.IOEvidence):
    """pipeline.py:751-755: the pose part of (PSD(L_pred + L_io) + eps_lift I)^-1 (h_pred + h_io)."""
    L_f = O.psd_project(bpred.L + io.L)[0]
    return O.chol_solve_lifted(L_f, bpred.h + io.h)[0][0:6]


def eps_lift_evidence(H=None):
    """The evidence of a scan without a map branch (pipeline.py:1014-1015): eps_lift I, 0."""
    L, h = O.EPS_LIFT * np.eye(O.D_Z), np.zeros(O.D_Z)
    return (L, h) if H is None else (np.tile(L, (H, 1, 1)), np.tile(h, (H, 1)))


def front(b_prev: O.Belief, scan: O.ScanInput, Q, io=None, Sigma_ga=None):
    """Predict, the IMU windows and preintegration, the measurement-IW statistics and (io=None) the
    IMU/odom branch: O.scan_hypothesis up to its bin path, statement for statement."""
    bud = O.point_budget_resample(scan.points, scan.timestamps, scan.weights, scan.ring, scan.tag,
                                  scan.points.shape[0])
    bpred, pc = O.predict_diffusion(b_prev, Q, scan.dt_sec)
    Sig_pred = O.chol_inverse_lifted(bpred.L)[0]
    sigma_warp = max(math.sqrt(Sig_pred[15, 15]), 0.01)
    w_scan = O.smooth_window_weights(scan.imu_stamps, scan.scan_start, scan.scan_end, sigma_warp)
    w_int = O.smooth_window_weights(scan.imu_stamps, scan.t_last, scan.t_scan, sigma_warp)
    mu_inc = O.chol_solve_lifted(bpred.L, bpred.h)[0]
    bg, ba = mu_inc[9:12], mu_inc[12:15]
    pose0 = O.world_pose(b_prev)
    rv0 = pose0[3:6]
    pre = O.preintegrate(scan.imu_stamps, scan.imu_gyro, scan.imu_accel, w_scan, rv0, bg, ba)
    xi = O.se3_log(pre["delta_pose"])
    dt_imu = O.imu_dt_mean(scan.imu_stamps)
    wv = w_int * (scan.imu_stamps > 0.0)
    wnv = wv / (np.sum(wv) + O.EPS_MASS)
    omega_avg = np.einsum("m,mi->i", wnv, scan.imu_gyro - bg[None, :])
    dPsi_meas = np.zeros((3, 3, 3))
    dPsi_meas[0] = O.iw_meas_gyro_suffstats(scan.imu_gyro, wv, bg, omega_avg, dt_imu)
    dPsi_meas[1] = O.iw_meas_accel_suffstats(rv0, scan.imu_accel, wv, ba, dt_imu)
    io_parts = None
    if io is None:
        pre_int = O.preintegrate(scan.imu_stamps, scan.imu_gyro, scan.imu_accel, w_int, rv0, bg, ba)
        dt_int = O.imu_integration_time(scan.imu_stamps, scan.t_last, scan.t_scan)
        io, io_parts = O.imu_odom_branch(b_prev, bpred, scan.odom, scan.imu_accel, scan.imu_gyro, w_int, ba, pre_int,
                                         dt_int, dt_imu, omega_avg, scan.dt_sec, Sigma_ga[0], Sigma_ga[1])
    return dict(bud=bud, bpred=bpred, pc=pc, pre=pre, xi=xi, dPsi_meas=dPsi_meas, io=io, io_parts=io_parts)


def scan_hypothesis_given(b_prev: O.Belief, scan: O.ScanInput, Q, io, L_lidar, h_lidar, lidar_cert, Sigma_ga=None):
    """One hypothesis of a scan whose LiDAR evidence is given. io=None: the IMU/odom branch is computed
    from scan.odom and the IMU window with Sigma_ga = (Sigma_g, Sigma_a), as O.scan_hypothesis does."""
    f = front(b_prev, scan, Q, io, Sigma_ga)
    bud, bpred, pc, xi, dPsi_meas, io, io_parts = (f[k] for k in ("bud", "bpred", "pc", "xi", "dPsi_meas", "io",
                                                                   "io_parts"))
    dnu_meas = np.array([1.0, 1.0, 0.0])
    zlin = z_lin_pose(bpred, io)
    # ---- pipeline.py:1038-1067
    L_raw = io.L + np.asarray(L_lidar, np.float64)
    h_raw = io.h + np.asarray(h_lidar, np.float64)
    lc = lidar_cert
    ess_tot = (float(lc[0]) + io.ess.sum()) / 4.0
    sf_tot = (float(lc[1]) + io.support.sum()) / 4.0
    exc_total = max(0.0, max(float(lc[3]), io.exc_dt)) + max(0.0, max(float(lc[4]), io.exc_ex))
    nll = float(lc[2]) + io.nll
    # ---- :1070-1206
    beta, dt_asym, z_xy = O.tempering_beta(L_raw, ess_tot, exc_total)
    L_ev, h_ev = beta * L_raw, beta * h_raw
    Lps, hps, s_dt, s_ex = O.excitation_scaling(L_ev, bpred.L, bpred.h)
    cond6 = O.pose6_cond(L_ev)
    alpha = O.fusion_alpha(cond6, ess_tot, exc_total, dt_asym, z_xy, beta, nll)
    L_post, h_post, fc = O.info_fusion_additive(Lps, hps, L_ev, h_ev, alpha)
    # ---- :1211
    T = bud["trig"] + pc["trig"] + io.trig
    for v in np.atleast_1d(np.asarray(lc[5], np.float64)):
        T = T + float(v)
    T = (T + O.trigger(beta=beta) + O.trigger(dt=1.0 - s_dt, ex=1.0 - s_ex) + O.trigger(alpha=alpha)
         + O.trigger(psd=fc[0], alpha=alpha))
    b_post = O.Belief(bpred.X_anchor.copy(), bpred.z_lin.copy(), L_post, h_post, bpred.stamp_sec)
    b_rec, rc = O.recompose(b_post, T)
    dPsi_p, dnu_p = O.iw_process_suffstats(Lps, hps, b_rec.L, b_rec.h)
    z_t = O.world_pose(b_rec)  # :1244, the pose of step 12b
    Sig_pose = O.chol_inverse_lifted(b_rec.L)[0][0:6, 0:6]
    b_fin, dr = O.anchor_drift(b_rec)
    return dict(belief=b_fin, dPsi_proc=dPsi_p, dnu_proc=dnu_p, dPsi_meas=dPsi_meas, dnu_meas=dnu_meas,
                T=T, beta=beta, alpha=alpha, s_dt=s_dt, s_ex=s_ex, xi_body=xi, rho=dr["rho"],
                frob=rc["frobenius_strength"], pose=O.world_pose(b_fin), L_post=L_post, h_post=h_post, io=io,
                io_parts=io_parts, L_ev=L_ev, cond6=cond6, eigmin6=O.pose6_eigs(L_ev)[0], fc=np.asarray(fc),
                z_lin_pose=zlin, pose_pred=O.world_pose(bpred), z_t=z_t, Sig_pose=Sig_pose, ess_total=ess_tot,
                support_frac=sf_tot, exc_total=exc_total, nll=nll)


def process_scan_given(state: O.ScanState, scan: O.ScanInput, ios, L_lidar, h_lidar, lidar_certs):
    """backend_node.py:2036-2119 for H hypotheses of a given-evidence scan: O.process_scan without the
    bin map's update (the map is carried unchanged). lidar_certs: one row, or one per hypothesis."""
    H = len(state.beliefs)
    Q = O.iw_process_Q(state.nu_proc, state.Psi_proc)
    Sga = (O.iw_meas_mode(state.nu_meas, state.Psi_meas, 0), O.iw_meas_mode(state.nu_meas, state.Psi_meas, 1))
    certs = np.asarray(lidar_certs, np.float64)
    certs = np.tile(certs, (H, 1)) if certs.ndim == 1 else certs
    res = [scan_hypothesis_given(state.beliefs[i], scan, Q, None if ios is None else ios[i], L_lidar[i], h_lidar[i],
                                 certs[i], Sga) for i in range(H)]
    aP = np.zeros((7, 6, 6)); an = np.zeros(7); aM = np.zeros((3, 3, 3)); am = np.zeros(3)
    for i, r in enumerate(res):
        w = float(state.weights[i])
        aP = aP + w * r["dPsi_proc"]; an = an + w * r["dnu_proc"]
        aM = aM + w * r["dPsi_meas"]; am = am + w * r["dnu_meas"]
    nb = [r["belief"] for r in res]
    comb = O.hypothesis_barycenter(np.stack([b.L for b in nb]), np.stack([b.h for b in nb]),
                                   np.stack([b.z_lin for b in nb]), state.weights, 0.01 / H)
    wp = float(min(1, state.scan_count))
    nu_p, Psi_p, _ = O.iw_process_apply(state.nu_proc, state.Psi_proc, wp * aP, wp * an)
    nu_m, Psi_m, _ = O.iw_meas_apply(state.nu_meas, state.Psi_meas, aM, am)
    st = O.ScanState(nb, state.weights.copy(), nu_p, Psi_p, nu_m, Psi_m, state.map, state.scan_count + 1)
    return st, comb, res

