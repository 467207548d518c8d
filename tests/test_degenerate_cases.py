"""The degenerate-scan cases of tests/test_gpu_degenerate_scans.py (oracle/cases.DEGENERATE: the node's
first scan on an empty map, scans with all / half of the weights zero, planar and corridor geometry) are
well-posed in the oracle: three chained scans of process_scan at the GPU test's size (H = 3, 4,096 points),
unperturbed against the points scaled by 1 ± 2^-52, move every compared quantity by at most a tenth of its
bar in test_gpu_configs._run_and_compare and change no near-null count (no clamp decision rides on
rounding). Parity at those bars is then a fair demand of the kernels.

T, the sum over every certificate magnitude, is the one field that is sensitive (~1e-8 relative) while the
reference's ~1e-16 ||M|| rounding of inactive clamps' deltas is in it; with those deltas exact (O.exact_inactive_deltas, as
_run_and_compare runs the oracle) it stays within a tenth of its 1e-10 bar in every case, so no case
needs a looser T."""

import numpy as np
import pytest

from oracle import cases
from oracle import gc_oracle as O

H, N_AZ, N_SCANS = 3, 256, 3
EPS_LIFT = 1e-9

# field -> (rel, abs) of _run_and_compare
BARS = {
    "xi_body": (1e-9, 1e-12), "bin N": (1e-10, 0.0), "bin s_dir": (1e-10, 0.0), "bin p_bar": (1e-10, 1e-12),
    "Sigma_p": (1e-7, 1e-12), "avg entropy": (1e-9, 0.0), "R_mf": (1e-7, 1e-10), "t_wls": (1e-7, 1e-10),
    "T": (1e-10, 1e-12), "MF trigger": (0.0, 1e-9), "planar trigger": (0.0, 1e-9), "alpha": (0.0, 1e-12),
    "excitation scales": (0.0, 1e-12), "cond_pose6": (1e-6, 0.0), "moment psd delta": (0.0, 1e-10),
    "moment mass-eps ratio": (1e-8, 1e-300), "moment trigger": (0.0, 1e-10), "beta": (0.0, 1e-10),
    "world pose": (0.0, 1e-6), "X_anchor": (0.0, 1e-6), "L": (1e-8, 0.0), "z_lin": (1e-6, 1e-9),
    "pose covariance": (0.0, 1e-6), "covariance": (1e-8, 0.0), "dPsi_proc": (1e-8, 1e-18),
    "dPsi_meas": (1e-8, 1e-18), "combined L": (1e-10, 0.0), "combined h": (1e-10, 1e-12),
    "combined z_lin": (1e-10, 1e-12), "Psi_proc": (1e-9, 1e-20), "Psi_meas": (1e-9, 1e-20), "Q": (1e-9, 1e-20),
    "map": (1e-8, 1e-12),
}


def _cov(L):
    return np.linalg.inv(L + EPS_LIFT * np.eye(L.shape[-1]))


def _fields(r):
    b = r["belief"]
    S = _cov(b.L)
    return {
        "xi_body": r["xi_body"], "bin N": r["moments"]["N"], "bin s_dir": r["moments"]["s_dir"],
        "bin p_bar": r["moments"]["p_bar"], "Sigma_p": r["moments"]["Sigma_p"],
        "avg entropy": r["assign"]["avg_entropy"], "R_mf": O.so3_log(r["mf"]["R_mf"]), "t_wls": r["planar"]["t_wls"],
        "T": r["T"], "MF trigger": r["mf"]["trig"], "planar trigger": r["planar"]["trig"], "alpha": r["alpha"],
        "excitation scales": [r["s_dt"], r["s_ex"]], "cond_pose6": r["cond6"],
        "moment psd delta": r["moments"]["psd_delta"], "moment mass-eps ratio": r["moments"]["max_eps_ratio"],
        "moment trigger": r["moments"]["trig"], "beta": r["beta"], "world pose": r["pose"], "X_anchor": b.X_anchor,
        "L": b.L, "z_lin": b.z_lin, "pose covariance": S[0:6, 0:6], "covariance": S, "dPsi_proc": r["dPsi_proc"],
        "dPsi_meas": r["dPsi_meas"],
    }


def _certs(r):
    """Every cert_vec / ConditioningCert the GPU test compares: (name, [.., eig_min, eig_max, cond, nnc])."""
    out = [("predict", np.concatenate([[0, 0], r["pred_cond"]])), ("fusion", np.concatenate([[0, 0], r["fusion_cond"]])),
           ("MF", r["mf"]["psd_cert"]), ("planar", r["planar"]["psd_cert"])]
    return out + [(f"bin {b}", c) for b, c in enumerate(r["moments"]["psd_certs"])]


def _ratio(a, b, rel, abs_):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    err = float(np.max(np.abs(a - b)))
    bound = rel * max(float(np.max(np.abs(b))), 1e-300) + abs_
    return err / bound


def _run(case, factor):
    st = case["state"]
    st = O.ScanState([O.Belief(b.X_anchor.copy(), b.z_lin.copy(), b.L.copy(), b.h.copy(), b.stamp_sec)
                      for b in st.beliefs], st.weights.copy(), st.nu_proc, st.Psi_proc, st.nu_meas, st.Psi_meas,
                     st.map.copy(), 0)
    outs = []
    for s in case["scans"]:
        s = dict(s)
        s["points"] = s["points"] * factor
        with O.exact_inactive_deltas():
            st, comb, res = O.process_scan(st, cases.scan_input(s), None, case["bins"], case["cfg"])
        outs.append((st, comb, res))
    return outs


def sensitivity(name):
    """{field: worst (perturbed - unperturbed) / bar} over the scans, hypotheses and both perturbations."""
    case = cases.build(H=H, n_az=N_AZ, n_scans=N_SCANS, io="computed", **cases.DEGENERATE[name])
    assert case["n"] == 4096
    base = _run(case, 1.0)
    worst = {}
    for factor in (1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52):
        for (st0, c0, r0), (st1, c1, r1) in zip(base, _run(case, factor)):
            pairs = []
            for a, b in zip(r1, r0):
                fa, fb = _fields(a), _fields(b)
                pairs += [(k, fa[k], fb[k]) for k in fb]
                for (cn, ca), (_, cb) in zip(_certs(a), _certs(b)):
                    sc = max(abs(cb[3]), 1e-300)
                    assert ca[5] == cb[5], (name, cn, "near-null count", ca, cb)
                    for what, x, y, rel, ab in (("cert deltas", ca[0:2], cb[0:2], 0.0, 1e-12 * sc),
                                                ("cert eig_max", ca[3], cb[3], 1e-10, 0.0),
                                                ("cert eig_min", ca[2], cb[2], 0.0, 1e-12 * sc)):
                        worst[what] = max(worst.get(what, 0.0), _ratio(x, y, rel, ab))
            pairs += [("combined L", c1["L"], c0["L"]), ("combined h", c1["h"], c0["h"]),
                      ("combined z_lin", c1["z_lin"], c0["z_lin"]), ("Psi_proc", st1.Psi_proc, st0.Psi_proc),
                      ("Psi_meas", st1.Psi_meas, st0.Psi_meas),
                      ("Q", O.iw_process_Q(st1.nu_proc, st1.Psi_proc), O.iw_process_Q(st0.nu_proc, st0.Psi_proc)),
                      ("map", cases.map_to_record(st1.map), cases.map_to_record(st0.map))]
            assert c1["psd_cert"][5] == c0["psd_cert"][5]
            for k, a, b in pairs:
                worst[k] = max(worst.get(k, 0.0), _ratio(a, b, *BARS[k]))
    return worst


@pytest.mark.parametrize("name", list(cases.DEGENERATE))
def test_degenerate_cases_are_well_posed(name):
    worst = sensitivity(name)
    for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:6]:
        print(f"{name}: {k} moves by {v:.3g} of its bar")
    loose = [k for k, v in worst.items() if v > 0.1]
    assert set(BARS) <= set(worst) and not loose, (name, {k: worst[k] for k in loose})
