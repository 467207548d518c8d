#!/usr/bin/env python3
"""Generate tests/golden/psd_edges.npz (TEST INFRASTRUCTURE): symmetric matrices at the edges of the
spectrum for the PSD projection and its ConditioningCert (domain_projection_psd_core,
primitives.py:80-123), with their eigenvalues and clamped reconstruction in 60-digit arithmetic, so
tests/test_gpu_psd_edges.py compares the HIP kernels with something better than another f64 eigh.

Per case: the f64 matrix M (= Q diag(λ) Qᵀ rounded, Q from a seeded QR; family h adds a skew part), the
eigenvalues of the STORED f64 symmetrised matrix 0.5 (M + Mᵀ) by mpmath.eigsy at 60 digits, the
projection Q diag(max(λ, ε)) Qᵀ from the mp eigenpairs rounded to f64, and the two deltas
[||M_psd − M_sym||_F, ||M_sym − M||_F] from the mp values.

Families (d = 22 unless noted; see FAMILIES):
  a  graded geomspace spectrum, cond 1e8 / 1e10 / 1e12          (d = 22, 6, 3, 23)
  b  two clusters, 11 x 1e-5 and 11 x 1e5                       (repeated eigenvalues)
  c  tiny, clamp inactive: 2e-12, 5e-12, 9e-12, 2e-11, geomspace(1e-10, 1e-9)   (d = 22, 6, 3)
  d  c with two eigenvalues replaced by 0.5e-12 and -3e-12      (d = 22, 6, 3, 23)
  e  exactly diagonal, unsorted: c I, the zero matrix, one entry below ε
  f  block-diagonal 6 + 16 with exact-zero coupling (clamp inactive / active)
  g  rank-1 s v vᵀ; negative definite                           (d = 22, 6, 3)
  h  a (cond 1e8) plus a skew part K: sym_delta = ||K||_F
  i  O(1) SPD diagonal blocks with couplings of 1e-160

check() (numpy only; tests/test_psd_edges_fixture.py runs it on the committed npz) asserts per case
  * every eigenvalue lies further than 1e3 d 2^-52 max|λ| from ε = 1e-12 and from 10 ε, so the clamp set
    and the near-null count do not depend on rounding;
  * numpy.linalg.eigh meets every bar the GPU test applies (BARS) against the mp values.

Needs mpmath to generate (about 10 s). Run from the repo root:  python tests/golden/make_psd_edges.py
"""

from __future__ import annotations

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NPZ = os.path.join(HERE, "psd_edges.npz")
EPS = 1e-12
SIZES = (22, 6, 3, 23)


def _q(rng, d):
    return np.linalg.qr(rng.normal(size=(d, d)))[0]


def _from_spectrum(rng, lam):
    lam = np.asarray(lam, np.float64)
    Q = _q(rng, lam.shape[0])
    M = (Q * lam) @ Q.T
    return 0.5 * (M + M.T)


def _tiny(d, active):
    small = [2e-12, 5e-12, 9e-12, 2e-11][:min(4, d - 1)]
    if active:
        small[0:2] = [0.5e-12, -3e-12]
    return np.array(small + list(np.geomspace(1e-10, 1e-9, d - len(small)) if d - len(small) > 1 else [1e-9]))


def _blockdiag(*blocks):
    d = sum(b.shape[0] for b in blocks)
    M = np.zeros((d, d))
    o = 0
    for b in blocks:
        M[o:o + b.shape[0], o:o + b.shape[0]] = b
        o += b.shape[0]
    return M


def families():
    """[(name, M)] in a fixed order; every matrix from its own seeded generator."""
    out = []
    seed = [1000]

    def rng():
        seed[0] += 1
        return np.random.default_rng(seed[0])

    for d in SIZES:
        for cond, lmax in ((1e8, 1e4), (1e10, 1e4), (1e12, 1e-2)):
            out.append((f"a_cond{cond:.0e}_d{d}", _from_spectrum(rng(), np.geomspace(lmax / cond, lmax, d))))
    out.append(("b_clusters_d22", _from_spectrum(rng(), [1e-5] * 11 + [1e5] * 11)))
    for d in (22, 6, 3):
        out.append((f"c_tiny_inactive_d{d}", _from_spectrum(rng(), _tiny(d, False))))
    for d in SIZES:
        out.append((f"d_tiny_active_d{d}", _from_spectrum(rng(), _tiny(d, True))))
    out.append(("e_cI_d22", 3.7 * np.eye(22)))
    out.append(("e_zero_d22", np.zeros((22, 22))))
    dg = rng().uniform(1e-3, 5e-2, 22)
    dg[7] = 0.0
    out.append(("e_diag_one_below_eps_d22", np.diag(dg)))
    r = rng()
    out.append(("f_blocks_inactive_d22", _blockdiag(_from_spectrum(r, np.geomspace(1e-2, 1.0, 6)),
                                                     _from_spectrum(r, np.geomspace(1e-1, 1e1, 16)))))
    r = rng()
    out.append(("f_blocks_active_d22", _blockdiag(_from_spectrum(r, [-0.5, 1e-2, 0.1, 0.3, 0.6, 1.0]),
                                                   _from_spectrum(r, np.geomspace(1e-1, 1e1, 16)))))
    for d in (22, 6, 3):
        r = rng()
        v = r.normal(size=d)
        v /= np.linalg.norm(v)
        out.append((f"g_rank1_d{d}", 0.1 * np.outer(v, v)))
        out.append((f"g_negdef_d{d}", -_from_spectrum(r, np.geomspace(1e-3, 1e-1, d))))
    r = rng()
    S = _from_spectrum(r, np.geomspace(1e-4, 1e4, 22))
    K = r.normal(size=(22, 22)) * 10.0
    out.append(("h_skew_d22", S + (K - K.T)))
    r = rng()
    M = _blockdiag(_from_spectrum(r, np.geomspace(0.1, 10.0, 11)), _from_spectrum(r, np.geomspace(0.2, 5.0, 11)))
    C = 1e-160 * r.uniform(0.5, 2.0, (11, 11))
    M[0:11, 11:22], M[11:22, 0:11] = C, C.T
    out.append(("i_blocks_1e-160_d22", M))
    r = rng()
    C = 1e-160 * r.uniform(0.5, 2.0, (22, 22))
    M = 0.5 * (C + C.T)
    M[np.diag_indices(22)] = r.uniform(0.5, 4.0, 22)
    out.append(("i_diag_1e-160_d22", M))
    return out


def make():
    import mpmath as mp
    mp.mp.dps = 60
    per = {d: [] for d in SIZES}
    eps = mp.mpf(EPS)
    for name, M in families():
        d = M.shape[0]
        Ms = 0.5 * (M + M.T)  # the f64 symmetrisation every kernel forms (exact sum, exact halving)
        E, Q = mp.eigsy(mp.matrix(Ms.tolist()))
        lam = [E[i] for i in range(d)]
        order = sorted(range(d), key=lambda i: lam[i])
        lc = [max(l, eps) for l in lam]
        Mp = np.array([[float(mp.fsum(Q[i, k] * lc[k] * Q[j, k] for k in range(d))) for j in range(d)]
                       for i in range(d)])
        proj = mp.sqrt(mp.fsum((lc[k] - lam[k]) ** 2 for k in range(d)))
        sym = mp.sqrt(mp.fsum((mp.mpf(float(Ms[i, j])) - mp.mpf(float(M[i, j]))) ** 2
                              for i in range(d) for j in range(d)))
        per[d].append((name, M, np.array([float(lam[i]) for i in order]), Mp, np.array([float(proj), float(sym)])))
        print(f"{name}: λ in [{float(lam[order[0]]):.3e}, {float(lam[order[-1]]):.3e}] delta {float(proj):.3e}")
    arrs = {}
    for d, cs in per.items():
        arrs[f"names_d{d}"] = np.array([c[0] for c in cs])
        for j, key in enumerate(("M", "lam", "Mp", "delta"), start=1):
            arrs[f"{key}_d{d}"] = np.stack([c[j] for c in cs])
    np.savez_compressed(NPZ, **arrs)
    print("wrote", NPZ, os.path.getsize(NPZ), "bytes")


def load(path=NPZ):
    """{d: [dict(name, M, lam, Mp, delta, cert)]}; cert = the reference cert_vec [projection_delta,
    sym_delta, eig_min, eig_max, cond, near_null_count] from the mp eigenvalues."""
    g = np.load(path)
    out = {}
    for d in SIZES:
        out[d] = []
        for k, name in enumerate(g[f"names_d{d}"]):
            lam = g[f"lam_d{d}"][k]
            lc = np.maximum(lam, EPS)
            cert = np.array([g[f"delta_d{d}"][k, 0], g[f"delta_d{d}"][k, 1], lc.min(), lc.max(), lc.max() / lc.min(),
                             float(np.sum(lc < 10.0 * EPS))])
            out[d].append(dict(name=str(name), M=g[f"M_d{d}"][k], lam=lam, Mp=g[f"Mp_d{d}"][k],
                               delta=g[f"delta_d{d}"][k], cert=cert))
    return out


def cond_rel_bound(cond):
    """What the eig_max (1e-10 relative) and eig_min (1e-12 eig_max absolute) bars leave for cond."""
    return 2.0 * (1e-12 * float(cond) + 1e-10)


def bars(case, Mp, cert):
    """The GPU test's bars for one case: [(what, error, bound)] of a projection Mp (or None) and its
    cert_vec [projection_delta, sym_delta, eig_min, eig_max, cond, near_null_count] (NaN delta entries
    are skipped by the caller) against the mp values. The project's bars of _cond_fields / _cert6."""
    ref = case["cert"]
    d = case["M"].shape[0]
    # the deltas' scale: the size of what they are differences of, ||M_sym||_2 = max|λ| before the clamp,
    # eig_max after it (_cert6's scale; the two agree unless the largest |λ| is negative) and max|M_ij|
    # (the skew part of family h enters sym_delta alone)
    sc = max(ref[3], np.max(np.abs(case["lam"])), np.max(np.abs(case["M"])))
    out = [("eig_max", abs(cert[3] - ref[3]), 1e-10 * ref[3]),
           ("eig_min", abs(cert[2] - ref[2]), 1e-12 * ref[3]),
           ("near-null count", abs(cert[5] - ref[5]), 0.0),
           ("cond (own extremes)", abs(cert[4] - cert[3] / cert[2]), 1e-15 * cert[4]),
           ("projection delta", abs(cert[0] - ref[0]), 1e-12 * sc),
           ("sym delta", abs(cert[1] - ref[1]), 1e-12 * sc)]
    rel = cond_rel_bound(ref[4])
    if rel < 0.5:
        out.append(("cond", abs(cert[4] - ref[4]), rel * ref[4]))
    if Mp is not None:
        scale = max(np.max(np.abs(case["M"])), np.max(np.abs(case["Mp"])))
        out.append(("M_psd", float(np.max(np.abs(Mp - case["Mp"]))), 1e-12 * scale * max(1.0, d / 16.0)))
    return out


def eigh_projection(M, eps=EPS):
    """domain_projection_psd_core in numpy f64 (primitives.py:80-123)."""
    Ms = 0.5 * (M + M.T)
    w, V = np.linalg.eigh(Ms)
    wc = np.maximum(w, eps)
    Mp = (V * wc) @ V.T
    cert = np.array([np.linalg.norm(Mp - Ms), np.linalg.norm(Ms - M), wc.min(), wc.max(), wc.max() / wc.min(),
                     float(np.sum(wc < 10.0 * eps))])
    return Mp, cert


def check(path=NPZ):
    """The fixture's own conditions (module docstring); returns the worst eigh error / bound ratio."""
    worst = 0.0
    n = 0
    for d, cs in load(path).items():
        for c in cs:
            lam = c["lam"]
            margin = 1e3 * d * 2.0 ** -52 * np.max(np.abs(lam))
            for thr in (EPS, 10.0 * EPS):
                assert np.all(np.abs(lam - thr) > margin), (c["name"], thr, margin, lam)
            assert np.all(np.isfinite(c["M"])) and np.all(np.isfinite(c["Mp"]))
            Mp, cert = eigh_projection(c["M"])
            for what, err, bound in bars(c, Mp, cert):
                assert err <= bound, (c["name"], what, err, bound)
                if bound > 0.0:
                    worst = max(worst, err / bound)
            n += 1
    return n, worst


if __name__ == "__main__":
    make()
    print("cases %d, worst eigh error / bar %.3g" % check())
